// Host side of the MI355X RNN resampler: the pf_rnn_* entries of include/pf_engine.h.
//
// Turns one resampling of models/DPF_RNN_resampling.py (rnn.py:263-349, or the baseline of
// rnn.py:217-261) for B problems into a stream-ordered sequence of launches of pf_rnn_kernels.h:
// upload, the input projection, the recurrence (one launch whatever N is), the assignment, download.
// pf_rnn_backward runs the same launches in the recording variant and then the backward chain of
// pf_rnn_kernels.h, in a workspace (pf_rnn_bwd_plan.h) its first call allocates.
// pf_rnn_set_weights repacks the Keras arrays into the padded slot layout and the MFMA fragments of
// pf_rnn_plan.h; pf_rnn_set_weights_dev does the same on the device (k_rnn_pack).  The launches of
// each pass are one enqueue_* function on device pointers and a stream: the host entries call it on
// the handle's staging buffers and stream, between their copies, the *_dev entries on the caller's
// pointers and stream, with no copies.
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "../../include/pf_engine.h"
#include "pf_dpf_host.h"
#include "pf_rnn_bwd_plan.h"
#include "pf_rnn_kernels.h"
#include "pf_rnn_plan.h"

using namespace pf::rnn;
namespace dpf = pf::dpf;
using pf::DevBuf;
using pf::fail;

// what the first pf_rnn_backward of a handle allocates
struct RnnBwd {
  BwdPlan plan{};
  bool fragT_current = false;  // the transposed fragments are those of the handle's weights
  DevBuf<double> hist_h, hist_c, dz, fragT, part, S, w0i, k0x, dense, gz, gXo, gX, ghid, gw, out;
};

struct pf_rnn_handle {
  int N = 0, d = 0, B = 0, H = 0, L = 0, cell = 0, use_weight = 0, use_particle = 0, device = 0;
  Plan plan{};
  bool have_weights = false;
  pf::Stream stream;  // before the buffers: destroyed after them
  dpf::Fence fence;   // orders the entries, which may run on different streams
  DevBuf<double> Xin, win, P, W0x, W0i, binit, frag, Kd, bd, hid, A, Xout;
  std::unique_ptr<RnnBwd> bwd;
  ~pf_rnn_handle() { dpf::quiesce(device, stream, fence); }
};

namespace {

template <int CELL, int L, bool RES>
hipError_t launch_recur_inst(dim3 grid, dim3 block, size_t lds, hipStream_t s, const RecurArgs& a) {
  if (a.rec_h) {  // the recording variant of pf_rnn_backward
    const hipError_t e = hipFuncSetAttribute((const void*)k_rnn_recur<CELL, L, RES, true>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((k_rnn_recur<CELL, L, RES, true>), grid, block, lds, s, a);
    return hipSuccess;
  }
  const hipError_t e = hipFuncSetAttribute((const void*)k_rnn_recur<CELL, L, RES>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_rnn_recur<CELL, L, RES>), grid, block, lds, s, a);
  return hipSuccess;
}

template <int CELL, int L, bool RES>
hipError_t launch_bwd_inst(dim3 grid, dim3 block, size_t lds, hipStream_t s, const BwdRecurArgs& a) {
  const hipError_t e = hipFuncSetAttribute((const void*)k_rnn_bwd_recur<CELL, L, RES>,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((k_rnn_bwd_recur<CELL, L, RES>), grid, block, lds, s, a);
  return hipSuccess;
}

template <int CELL, bool RES>
hipError_t launch_bwd_l(int L, dim3 grid, dim3 block, size_t lds, hipStream_t s, const BwdRecurArgs& a) {
  switch (L) {
    case 1: return launch_bwd_inst<CELL, 1, RES>(grid, block, lds, s, a);
    case 2: return launch_bwd_inst<CELL, 2, RES>(grid, block, lds, s, a);
    case 3: return launch_bwd_inst<CELL, 3, RES>(grid, block, lds, s, a);
    default: return launch_bwd_inst<CELL, 4, RES>(grid, block, lds, s, a);
  }
}

hipError_t launch_bwd_recur(const pf_rnn_handle* h, hipStream_t s, const BwdRecurArgs& a) {
  const dim3 grid(h->plan.tiles, h->B), block(h->plan.threads);
  const size_t lds = h->bwd->plan.lds_bytes;
  const bool res = h->bwd->plan.resident;
  if (h->cell == CELL_LSTM)
    return res ? launch_bwd_l<CELL_LSTM, true>(h->L, grid, block, lds, s, a)
               : launch_bwd_l<CELL_LSTM, false>(h->L, grid, block, lds, s, a);
  return res ? launch_bwd_l<CELL_GRU, true>(h->L, grid, block, lds, s, a)
             : launch_bwd_l<CELL_GRU, false>(h->L, grid, block, lds, s, a);
}

template <int CELL, bool RES>
hipError_t launch_recur_l(int L, dim3 grid, dim3 block, size_t lds, hipStream_t s, const RecurArgs& a) {
  switch (L) {
    case 1: return launch_recur_inst<CELL, 1, RES>(grid, block, lds, s, a);
    case 2: return launch_recur_inst<CELL, 2, RES>(grid, block, lds, s, a);
    case 3: return launch_recur_inst<CELL, 3, RES>(grid, block, lds, s, a);
    default: return launch_recur_inst<CELL, 4, RES>(grid, block, lds, s, a);
  }
}

hipError_t launch_recur(const pf_rnn_handle* h, hipStream_t s, const RecurArgs& a) {
  const dim3 grid(h->plan.tiles, h->B), block(h->plan.threads);
  const size_t lds = h->plan.lds_bytes;
  if (h->cell == CELL_LSTM)
    return h->plan.resident ? launch_recur_l<CELL_LSTM, true>(h->L, grid, block, lds, s, a)
                            : launch_recur_l<CELL_LSTM, false>(h->L, grid, block, lds, s, a);
  return h->plan.resident ? launch_recur_l<CELL_GRU, true>(h->L, grid, block, lds, s, a)
                          : launch_recur_l<CELL_GRU, false>(h->L, grid, block, lds, s, a);
}

// the slot a gate of the input kernel (rec = false) or the recurrent kernel (rec = true) feeds
int slot_of(int cell, int gate, bool rec) { return (cell == CELL_GRU && rec && gate == 2) ? 3 : gate; }

hipError_t upload(DevBuf<double>& buf, const std::vector<double>& v, hipStream_t s) {
  return hipMemcpyAsync(buf, v.data(), v.size() * sizeof(double), hipMemcpyHostToDevice, s);
}

// the handle was made under the test hook PF_TEST_RNN_STREAM: the backward recurrence streams as well
bool force_streamed(const pf_rnn_handle* h) {
  return !h->plan.resident && make_plan(h->N, h->d, h->H, h->L, h->cell, h->use_weight, h->use_particle).resident;
}

// the workspace of the backward pass, on the first call
pf_status ensure_bwd(pf_rnn_handle* h) {
  if (h->bwd) return PF_OK;
  std::unique_ptr<RnnBwd> w(new RnnBwd());
  w->plan = make_bwd_plan(h->plan, h->N, h->d, h->B, h->H, h->L, h->cell, force_streamed(h));
  const BwdPlan& q = w->plan;
  const size_t BN = (size_t)h->B * h->N;
  if (pf_status st = dpf::alloc_all(
          {{&w->hist_h, q.hist_doubles}, {&w->dz, q.dz_doubles}, {&w->fragT, h->plan.frag_doubles},
           {&w->part, q.part_doubles}, {&w->S, q.sums_doubles}, {&w->w0i, q.w0i_doubles}, {&w->k0x, q.k0x_doubles},
           {&w->dense, q.dense_doubles}, {&w->gz, q.pair_doubles}, {&w->gXo, BN * h->d}, {&w->gX, BN * h->d},
           {&w->ghid, BN * h->H}, {&w->gw, BN}, {&w->out, q.out_doubles}},
          "backward workspace"))
    return st;
  if (q.c_doubles)
    if (pf_status st = dpf::alloc_all({{&w->hist_c, q.c_doubles}}, "backward workspace")) return st;
  h->bwd = std::move(w);
  return PF_OK;
}

// The transposed fragments from the forward's, which hold every entry of the padded matrices:
// fragment (tile, ks, slot) of the transposed set holds in lane l the entry (k, u) = (16 tile + (l & 15),
// 4 ks + (l >> 4)), which the forward's set keeps in fragment (u / 16, k / 4, slot), lane 16 (k % 4) + u % 16.
// Rows k >= 4 KS are rows of padded units: zero.
// Rows k >= 4 KS are rows of padded units: zero.  A permutation on the device (k_rnn_pack_T).
pf_status pack_transposed(pf_rnn_handle* h, hipStream_t s) {
  const Plan& p = h->plan;
  const int64_t n = (int64_t)p.frag_doubles;
  hipLaunchKernelGGL(k_rnn_pack_T, dim3((unsigned)((n + PB - 1) / PB)), dim3(PB), 0, s,
                     pack_net(p, h->N, h->H, h->L, h->cell), n, (const double*)h->frag, (double*)h->bwd->fragT);
  PF_HIPCHK(hipGetLastError());
  h->bwd->fragT_current = true;
  return PF_OK;
}

// the count and the sizes of the n = 3 L + 2 Keras arrays (`what`: "weight" or "gradient")
pf_status check_arrays(const pf_rnn_handle* h, const double* const* arrays, const int64_t* sizes, int32_t n,
                       const char* what, int64_t* want) {
  const int L = h->L;
  if (n != 3 * L + 2)
    return fail(PF_E_ARG, "expected " + std::to_string(3 * L + 2) + " " + what +
                              " arrays (3 per layer and 2 of the output layer)");
  keras_sizes(h->N, h->plan.F0, h->H, L, h->cell, want);
  for (int k = 0; k < n; ++k) {
    if (!arrays[k]) return fail(PF_E_ARG, std::string(what) + " array " + std::to_string(k) + " is null");
    if (sizes[k] != want[k])
      return fail(PF_E_ARG, std::string(what) + " array " + std::to_string(k) + " has " +
                                std::to_string((long long)sizes[k]) + " elements, expected " +
                                std::to_string((long long)want[k]));
  }
  return PF_OK;
}

// The launches of one resampling on stream s, every pointer device memory: X, w -> X_out, A, hid
// (rec_h, rec_c: the recording variant of the backward pass).
pf_status enqueue_resample(pf_rnn_handle* h, hipStream_t s, const dpf::Poison& poison, double temperature,
                           const double* X, const double* w, double* X_out, double* A, double* hid, double* rec_h,
                           double* rec_c) {
  const int N = h->N, d = h->d, B = h->B, H = h->H;
  const Plan& p = h->plan;
  const int W4 = SLOTS * p.Hp;
  const ProjArgs pa{N, d, W4, p.F0, h->use_weight, h->use_particle, X, w, h->W0x, h->binit, h->P};
  hipLaunchKernelGGL(k_rnn_project, dim3((W4 + PB - 1) / PB, N, B), dim3(PB), 0, s, pa);
  const RecurArgs ra{N, H, p.Hp, p.HT, p.KS, p.RS, h->P, h->W0i, h->binit, h->frag, p.frag_doubles, hid, rec_h, rec_c};
  poison();
  PF_HIPCHK(launch_recur(h, s, ra));
  AssignArgs aa{};
  aa.N = N, aa.d = d, aa.H = H;
  aa.hid = hid, aa.Kd = h->Kd, aa.bd = h->bd, aa.inv_T = 1.0 / temperature;
  aa.X = X, aa.A = A, aa.X_out = X_out;
  poison();
  hipLaunchKernelGGL(k_rnn_assign<false>, dim3(N, B), dim3(PB), 0, s, aa);
  return PF_OK;
}

// The launches of one backward pass on stream s, every pointer device memory.  The workspace holds
// grad_A (or zeros) in gz on entry; gX, gw and the n arrays of `outs` receive the gradients.
pf_status enqueue_backward(pf_rnn_handle* h, hipStream_t s, double temperature, const double* X, const double* w,
                           const double* gXo, double* gX, double* gw, double* const* outs, const int64_t* want,
                           int32_t n) {
  const int N = h->N, d = h->d, B = h->B, H = h->H, L = h->L;
  const Plan& p = h->plan;
  RnnBwd& w_ = *h->bwd;
  const BwdPlan& q = w_.plan;
  const int W4 = SLOTS * p.Hp;
  if (!w_.fragT_current) {
    if (pf_status st = pack_transposed(h, s)) return st;
  }
  PF_HIPCHK(hipMemsetAsync(gw, 0, (size_t)B * N * 8, s));  // stays 0 when use_weight = 0
  const dpf::Poison poison(s);  // tests only: in front of every launch that stages through LDS
  // the forward launches, recording
  if (pf_status st = enqueue_resample(h, s, poison, temperature, X, w, h->Xout, h->A, h->hid, w_.hist_h, w_.hist_c))
    return st;
  // the backward chain
  const BwdAssignArgs ba{N, d, H, X, gXo, h->A, h->Kd, 1.0 / temperature, w_.gz, w_.ghid};
  poison();
  hipLaunchKernelGGL(k_rnn_bwd_assign, dim3(N, B), dim3(PB), 0, s, ba);
  const BwdColsArgs ca{N, d, H, h->A, w_.gz, h->hid, gXo, w_.dense, gX};
  hipLaunchKernelGGL(k_rnn_bwd_cols, dim3((N + PB - 1) / PB, H + 1 + d, B), dim3(PB), 0, s, ca);
  const BwdRecurArgs br{N, H, p.Hp, p.HT, p.KS, p.RS, h->P, h->W0i, h->binit, h->frag, w_.fragT, p.frag_doubles,
                        w_.hist_h, w_.hist_c, w_.ghid, w_.dz};
  poison();
  PF_HIPCHK(launch_bwd_recur(h, s, br));
  const int nb = (W4 + PB - 1) / PB;
  const BwdSumArgs sa{N, L, p.Hp, p.tiles, p.F0, h->use_weight, w_.dz, X, w, h->W0x, d,
                      w_.S, w_.w0i, w_.k0x, gX, gw};
  hipLaunchKernelGGL(k_rnn_bwd_sums, dim3(L * nb, N, B), dim3(PB), 0, s, sa);
  hipLaunchKernelGGL(k_rnn_bwd_w0i, dim3(nb, N, B), dim3(PB), 0, s, sa);
  const BwdWgradArgs wa{N, L, p.Hp, p.HT, p.tiles, q.wg_tc, q.wg_chunks, q.mats, w_.hist_h, w_.dz, w_.part};
  hipLaunchKernelGGL(k_rnn_bwd_wgrad, dim3(p.HT * SLOTS * p.HT, q.wg_chunks * q.mats, B), dim3(64), 0, s, wa);
  hipLaunchKernelGGL(k_rnn_bwd_k0x, dim3(nb, p.F0, B), dim3(PB), 0, s, sa);
  hipLaunchKernelGGL(k_rnn_bwd_feat, dim3(p.F0, N, B), dim3(64), 0, s, sa);
  for (int k = 0; k < n; ++k) {
    BwdFinishArgs fa{};
    fa.kind = k < 3 * L ? k % 3 : 3 + (k - 3 * L);
    fa.l = k < 3 * L ? k / 3 : 0;
    fa.N = N, fa.H = H, fa.Hp = p.Hp, fa.F0 = p.F0, fa.B = B, fa.L = L, fa.cell = h->cell;
    fa.chunks = q.wg_chunks, fa.mats = q.mats;
    fa.part = w_.part, fa.S = w_.S, fa.w0i = w_.w0i, fa.k0x = w_.k0x, fa.dense = w_.dense;
    fa.out = outs[k], fa.count = want[k];
    hipLaunchKernelGGL(k_rnn_bwd_finish, dim3((unsigned)((want[k] + PB - 1) / PB)), dim3(PB), 0, s, fa);
  }
  PF_HIPCHK(hipGetLastError());
  return PF_OK;
}

}  // namespace

extern "C" {

pf_status pf_rnn_create(const pf_rnn_opts* o, pf_rnn_handle** out) try {
  if (!o || !out) return fail(PF_E_ARG, "null argument");
  *out = nullptr;
  if (pf_status st = dpf::check_shape(o->n_particles, false, o->dim)) return st;
  if (o->hidden < 1 || o->hidden > MAXH) return fail(PF_E_ARG, "hidden must be in 1 .. 128");
  if (o->layers < 1 || o->layers > MAXL) return fail(PF_E_ARG, "layers must be in 1 .. 4");
  if (pf_status st = dpf::check_batch(o->batch)) return st;
  if (o->cell != CELL_LSTM && o->cell != CELL_GRU) return fail(PF_E_ARG, "cell must be 0 (lstm) or 1 (gru)");
  if (!o->use_weight && !o->use_particle)
    return fail(PF_E_ARG, "use_weight and use_particle are both 0: at least one feature is needed");
  if (o->n_particles > MAXPAIRS || o->n_particles * o->n_particles > MAXPAIRS / o->batch)
    return fail(PF_E_ARG, "batch x n_particles^2 must be at most 2^28");

  PF_HIPCHK(hipSetDevice(o->device));
  std::unique_ptr<pf_rnn_handle> h(new pf_rnn_handle());
  const int N = h->N = (int)o->n_particles;
  const int d = h->d = o->dim, B = h->B = o->batch, H = h->H = o->hidden, L = h->L = o->layers;
  h->cell = o->cell;
  h->use_weight = o->use_weight ? 1 : 0;
  h->use_particle = o->use_particle ? 1 : 0;
  h->device = o->device;
  // tests only (pf_hooks.h): the streaming variant at any shape
  h->plan = make_plan(N, d, H, L, h->cell, h->use_weight, h->use_particle, pf::test_hook("PF_TEST_RNN_STREAM"));
  const Plan& p = h->plan;
  if (pf_status st = dpf::make_stream(h->stream)) return st;
  const size_t W4 = (size_t)SLOTS * p.Hp;
  if (pf_status st = dpf::alloc_all(
          {{&h->Xin, (size_t)B * N * d}, {&h->win, (size_t)B * N}, {&h->P, (size_t)B * N * W4},
           {&h->W0x, (size_t)p.F0 * W4}, {&h->W0i, (size_t)N * W4}, {&h->binit, (size_t)L * W4},
           {&h->frag, p.frag_doubles}, {&h->Kd, (size_t)H * N}, {&h->bd, (size_t)N}, {&h->hid, (size_t)B * N * H},
           {&h->A, (size_t)B * N * N}, {&h->Xout, (size_t)B * N * d}},
          "state"))
    return st;
  *out = h.release();
  return PF_OK;
} catch (...) { return pf::on_exception("pf_rnn_create"); }

void pf_rnn_destroy(pf_rnn_handle* h) { delete h; }

pf_status pf_rnn_set_weights(pf_rnn_handle* h, const double* const* arrays, const int64_t* sizes, int32_t n) try {
  if (!h || !arrays || !sizes) return fail(PF_E_ARG, "null argument");
  const int N = h->N, H = h->H, L = h->L, cell = h->cell;
  const Plan& p = h->plan;
  const int G = cell == CELL_LSTM ? 4 : 3, GH = G * H, Hp = p.Hp, W4 = SLOTS * Hp;
  int64_t want[3 * MAXL + 2];
  if (pf_status st = check_arrays(h, arrays, sizes, n, "weight", want)) return st;
  std::vector<double> W0x((size_t)p.F0 * W4, 0.0), W0i((size_t)N * W4, 0.0), binit((size_t)L * W4, 0.0),
      frag(p.frag_doubles, 0.0);
  for (int l = 0; l < L; ++l) {
    const double *K = arrays[3 * l], *R = arrays[3 * l + 1], *bias = arrays[3 * l + 2];
    for (int g = 0; g < G; ++g)
      for (int u = 0; u < H; ++u) {
        const size_t col = (size_t)slot_of(cell, g, false) * Hp + u;
        if (cell == CELL_LSTM) {
          binit[(size_t)l * W4 + col] = bias[g * H + u];
        } else if (g < 2) {
          binit[(size_t)l * W4 + col] = bias[g * H + u] + bias[3 * H + g * H + u];
        } else {
          binit[(size_t)l * W4 + col] = bias[g * H + u];
          binit[(size_t)l * W4 + (size_t)slot_of(cell, g, true) * Hp + u] = bias[3 * H + g * H + u];
        }
        if (l == 0) {
          for (int f = 0; f < p.F0; ++f) W0x[(size_t)f * W4 + col] = K[(size_t)f * GH + g * H + u];
          for (int i = 0; i < N; ++i) W0i[(size_t)i * W4 + col] = K[(size_t)(p.F0 + i) * GH + g * H + u];
        }
      }
    for (int which = (l == 0 ? 1 : 0); which < 2; ++which) {  // 0: input kernel, 1: recurrent kernel
      const double* M = which ? R : K;
      const int m = which ? 2 * l : 2 * l - 1;
      for (int tile = 0; tile < p.HT; ++tile)
        for (int ks = 0; ks < p.KS; ++ks)
          for (int g = 0; g < G; ++g) {
            double* f = frag.data() + frag_offset(p, m, tile, ks, slot_of(cell, g, which == 1));
            for (int lane = 0; lane < 64; ++lane) {
              const int k = 4 * ks + (lane >> 4), u = 16 * tile + (lane & 15);
              if (k < H && u < H) f[lane] = M[(size_t)k * GH + g * H + u];
            }
          }
    }
  }
  PF_HIPCHK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  PF_HIPCHK(h->fence.enter(s));
  const dpf::Fenced fenced{h->fence, s};
  h->have_weights = false;
  if (!W0x.empty()) PF_HIPCHK(upload(h->W0x, W0x, s));
  PF_HIPCHK(upload(h->W0i, W0i, s));
  PF_HIPCHK(upload(h->binit, binit, s));
  PF_HIPCHK(upload(h->frag, frag, s));
  PF_HIPCHK(hipMemcpyAsync(h->Kd, arrays[3 * L], (size_t)H * N * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(h->bd, arrays[3 * L + 1], (size_t)N * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipStreamSynchronize(s));  // the staging vectors go out of scope
  h->have_weights = true;
  if (h->bwd) h->bwd->fragT_current = false;  // repacked by the next pf_rnn_backward
  return PF_OK;
} catch (...) { return pf::on_exception("pf_rnn_set_weights"); }

pf_status pf_rnn_resample(pf_rnn_handle* h, const double* X, const double* w, double temperature, double* X_out,
                          double* A_out, double* hid_out) try {
  if (!h || !X || !w || !X_out) return fail(PF_E_ARG, "null argument");
  if (pf_status st = dpf::check_positive("temperature", temperature)) return st;
  if (!h->have_weights) return fail(PF_E_ARG, "pf_rnn_set_weights has not been called");
  PF_HIPCHK(hipSetDevice(h->device));
  const int N = h->N, d = h->d, B = h->B, H = h->H;
  hipStream_t s = h->stream;
  PF_HIPCHK(h->fence.enter(s));
  const dpf::Fenced fenced{h->fence, s};
  PF_HIPCHK(hipMemcpyAsync(h->Xin, X, (size_t)B * N * d * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(h->win, w, (size_t)B * N * 8, hipMemcpyHostToDevice, s));
  const dpf::Poison poison(s);  // tests only: in front of every launch that stages through LDS
  if (pf_status st = enqueue_resample(h, s, poison, temperature, h->Xin, h->win, h->Xout, h->A, h->hid, nullptr, nullptr))
    return st;
  PF_HIPCHK(hipGetLastError());
  PF_HIPCHK(hipMemcpyAsync(X_out, h->Xout, (size_t)B * N * d * 8, hipMemcpyDeviceToHost, s));
  if (A_out) PF_HIPCHK(hipMemcpyAsync(A_out, h->A, (size_t)B * N * N * 8, hipMemcpyDeviceToHost, s));
  if (hid_out) PF_HIPCHK(hipMemcpyAsync(hid_out, h->hid, (size_t)B * N * H * 8, hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipStreamSynchronize(s));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_rnn_resample"); }

pf_status pf_rnn_set_weights_dev(pf_rnn_handle* h, void* stream, const double* const* d_arrays, const int64_t* sizes,
                                 int32_t n) try {
  if (!h || !d_arrays || !sizes) return fail(PF_E_ARG, "null argument");
  int64_t want[3 * MAXL + 2];
  if (pf_status st = check_arrays(h, d_arrays, sizes, n, "weight", want)) return st;
  PF_HIPCHK(hipSetDevice(h->device));
  const Plan& p = h->plan;
  hipStream_t s = stream ? (hipStream_t)stream : (hipStream_t)h->stream;
  PF_HIPCHK(h->fence.enter(s));
  const dpf::Fenced fenced{h->fence, s};
  h->have_weights = false;
  PackArgs a{};
  a.net = pack_net(p, h->N, h->H, h->L, h->cell);
  for (int k = 0; k < n; ++k) a.src[k] = d_arrays[k];
  const int64_t W4 = (int64_t)SLOTS * p.Hp;
  a.W0x = h->W0x, a.W0i = h->W0i, a.binit = h->binit, a.frag = h->frag, a.Kd = h->Kd, a.bd = h->bd;
  a.n_W0x = p.F0 * W4, a.n_W0i = h->N * W4, a.n_binit = h->L * W4, a.n_frag = (int64_t)p.frag_doubles;
  a.n_Kd = (int64_t)h->H * h->N, a.n_bd = h->N;
  const int64_t all = a.n_W0x + a.n_W0i + a.n_binit + a.n_frag + a.n_Kd + a.n_bd;
  hipLaunchKernelGGL(k_rnn_pack, dim3((unsigned)((all + PB - 1) / PB)), dim3(PB), 0, s, a);
  PF_HIPCHK(hipGetLastError());
  h->have_weights = true;
  if (h->bwd) {  // the transposed set with the forward's, where a backward pass has run before
    if (pf_status st = pack_transposed(h, s)) return st;
  }
  if (!stream) PF_HIPCHK(hipStreamSynchronize(s));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_rnn_set_weights_dev"); }

pf_status pf_rnn_resample_dev(pf_rnn_handle* h, void* stream, const double* dX, const double* dw, double temperature,
                              double* dX_out, double* dA, double* d_hid) try {
  if (!h || !dX || !dw || !dX_out) return fail(PF_E_ARG, "null argument");
  if (pf_status st = dpf::check_positive("temperature", temperature)) return st;
  if (!h->have_weights) return fail(PF_E_ARG, "pf_rnn_set_weights has not been called");
  const size_t BN = (size_t)h->B * h->N;
  if (pf_status st = dpf::check_no_alias({{dX_out, BN * h->d}, {dA, BN * h->N}, {d_hid, BN * h->H}},
                                         {{dX, BN * h->d}, {dw, BN}}))
    return st;
  PF_HIPCHK(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : (hipStream_t)h->stream;
  PF_HIPCHK(h->fence.enter(s));
  const dpf::Fenced fenced{h->fence, s};
  const dpf::Poison poison(s);  // tests only, as in pf_rnn_resample
  if (pf_status st = enqueue_resample(h, s, poison, temperature, dX, dw, dX_out, dA ? dA : (double*)h->A,
                                      d_hid ? d_hid : (double*)h->hid, nullptr, nullptr))
    return st;
  PF_HIPCHK(hipGetLastError());
  if (!stream) PF_HIPCHK(hipStreamSynchronize(s));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_rnn_resample_dev"); }

pf_status pf_rnn_baseline(pf_rnn_handle* h, const double* X, const double* lp, uint64_t seed, uint32_t epoch,
                          uint32_t batch_base, double* X_out, double* A_out) try {
  if (!h || !X || !lp || !X_out) return fail(PF_E_ARG, "null argument");
  if (pf_status st = dpf::check_base(batch_base, h->B)) return st;
  PF_HIPCHK(hipSetDevice(h->device));
  const int N = h->N, d = h->d, B = h->B;
  hipStream_t s = h->stream;
  PF_HIPCHK(h->fence.enter(s));
  const dpf::Fenced fenced{h->fence, s};
  PF_HIPCHK(hipMemcpyAsync(h->Xin, X, (size_t)B * N * d * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(h->win, lp, (size_t)B * N * 8, hipMemcpyHostToDevice, s));
  AssignArgs aa{};
  aa.N = N, aa.d = d, aa.H = 0;
  aa.lp = h->win;
  aa.p = pf::soft::make_prob(N, d, B, seed, epoch, batch_base);
  aa.X = h->Xin, aa.A = h->A, aa.X_out = h->Xout;
  dpf::Poison{s}();  // tests only, as in pf_rnn_resample
  hipLaunchKernelGGL(k_rnn_assign<true>, dim3(N, B), dim3(PB), 0, s, aa);
  PF_HIPCHK(hipGetLastError());
  PF_HIPCHK(hipMemcpyAsync(X_out, h->Xout, (size_t)B * N * d * 8, hipMemcpyDeviceToHost, s));
  if (A_out) PF_HIPCHK(hipMemcpyAsync(A_out, h->A, (size_t)B * N * N * 8, hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipStreamSynchronize(s));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_rnn_baseline"); }

int64_t pf_rnn_backward_bytes(pf_rnn_handle* h) {
  if (!h) return 0;
  return (int64_t)make_bwd_plan(h->plan, h->N, h->d, h->B, h->H, h->L, h->cell, force_streamed(h)).workspace_bytes;
}

pf_status pf_rnn_backward(pf_rnn_handle* h, const double* X, const double* w, double temperature,
                          const double* grad_X_out, const double* grad_A, double* grad_X, double* grad_w,
                          double* const* grad_arrays, const int64_t* sizes, int32_t n) try {
  if (!h || !X || !w || !grad_X_out || !grad_X || !grad_w || !grad_arrays || !sizes) return fail(PF_E_ARG, "null argument");
  if (pf_status st = dpf::check_positive("temperature", temperature)) return st;
  if (!h->have_weights) return fail(PF_E_ARG, "pf_rnn_set_weights has not been called");
  const int N = h->N, d = h->d, B = h->B;
  int64_t want[3 * MAXL + 2];
  if (pf_status st = check_arrays(h, grad_arrays, sizes, n, "gradient", want)) return st;
  PF_HIPCHK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  if (pf_status st = ensure_bwd(h)) return st;
  PF_HIPCHK(h->fence.enter(s));
  const dpf::Fenced fenced{h->fence, s};
  RnnBwd& w_ = *h->bwd;
  const size_t nX = (size_t)B * N * d * 8, nA = (size_t)B * N * N * 8;
  PF_HIPCHK(hipMemcpyAsync(h->Xin, X, nX, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(h->win, w, (size_t)B * N * 8, hipMemcpyHostToDevice, s));
  PF_HIPCHK(hipMemcpyAsync(w_.gXo, grad_X_out, nX, hipMemcpyHostToDevice, s));
  if (grad_A)
    PF_HIPCHK(hipMemcpyAsync(w_.gz, grad_A, nA, hipMemcpyHostToDevice, s));
  else
    PF_HIPCHK(hipMemsetAsync(w_.gz, 0, nA, s));
  double* outs[3 * MAXL + 2];
  size_t off = 0;
  for (int k = 0; k < n; ++k) {
    outs[k] = w_.out + off;
    off += (size_t)want[k];
  }
  if (pf_status st = enqueue_backward(h, s, temperature, h->Xin, h->win, w_.gXo, w_.gX, w_.gw, outs, want, n)) return st;
  PF_HIPCHK(hipMemcpyAsync(grad_X, w_.gX, nX, hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipMemcpyAsync(grad_w, w_.gw, (size_t)B * N * 8, hipMemcpyDeviceToHost, s));
  for (int k = 0; k < n; ++k)
    PF_HIPCHK(hipMemcpyAsync(grad_arrays[k], outs[k], (size_t)want[k] * 8, hipMemcpyDeviceToHost, s));
  PF_HIPCHK(hipStreamSynchronize(s));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_rnn_backward"); }

pf_status pf_rnn_backward_dev(pf_rnn_handle* h, void* stream, const double* dX, const double* dw, double temperature,
                              const double* d_grad_X_out, const double* d_grad_A, double* d_grad_X, double* d_grad_w,
                              double* const* d_grad_arrays, const int64_t* sizes, int32_t n) try {
  if (!h || !dX || !dw || !d_grad_X_out || !d_grad_X || !d_grad_w || !d_grad_arrays || !sizes)
    return fail(PF_E_ARG, "null argument");
  if (pf_status st = dpf::check_positive("temperature", temperature)) return st;
  if (!h->have_weights) return fail(PF_E_ARG, "pf_rnn_set_weights has not been called");
  const int N = h->N, d = h->d, B = h->B;
  int64_t want[3 * MAXL + 2];
  if (pf_status st = check_arrays(h, d_grad_arrays, sizes, n, "gradient", want)) return st;
  const size_t BN = (size_t)B * N;
  const std::initializer_list<dpf::Span> ins = {{dX, BN * d}, {dw, BN}, {d_grad_X_out, BN * d}, {d_grad_A, BN * N}};
  if (pf_status st = dpf::check_no_alias({{d_grad_X, BN * d}, {d_grad_w, BN}}, ins)) return st;
  for (int k = 0; k < n; ++k)
    if (pf_status st = dpf::check_no_alias({{d_grad_arrays[k], (size_t)want[k]}}, ins)) return st;
  PF_HIPCHK(hipSetDevice(h->device));
  hipStream_t s = stream ? (hipStream_t)stream : (hipStream_t)h->stream;
  if (pf_status st = ensure_bwd(h)) return st;  // the first call allocates, which may wait for the device
  PF_HIPCHK(h->fence.enter(s));
  const dpf::Fenced fenced{h->fence, s};
  RnnBwd& w_ = *h->bwd;
  // k_rnn_bwd_assign turns grad_A into gz in place: the caller's stays the caller's
  if (d_grad_A)
    PF_HIPCHK(hipMemcpyAsync(w_.gz, d_grad_A, BN * N * 8, hipMemcpyDeviceToDevice, s));
  else
    PF_HIPCHK(hipMemsetAsync(w_.gz, 0, BN * N * 8, s));
  if (pf_status st = enqueue_backward(h, s, temperature, dX, dw, d_grad_X_out, d_grad_X, d_grad_w, d_grad_arrays, want, n))
    return st;
  if (!stream) PF_HIPCHK(hipStreamSynchronize(s));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_rnn_backward_dev"); }

int32_t pf_rnn_resident(pf_rnn_handle* h) { return (h && h->plan.resident) ? 1 : 0; }

void* pf_rnn_stream(pf_rnn_handle* h) { return dpf::stream_of(h); }

pf_status pf_rnn_synchronize(pf_rnn_handle* h) try {
  return dpf::synchronize(h);
} catch (...) { return pf::on_exception("pf_rnn_synchronize"); }

}  // extern "C"
