// Host side of the MI355X LEDH particle-flow filter: the C ABI of include/pf_ledh.h.
//
// Turns LEDHFlowPF's call sequence (/root/reference/models/LEDH_particle_filter.py:
// init_from_gaussian 84-91, step 93-214) into launches of pf_ledh_kernels.h, and runs
// the whole T loop on the device (pf_ledh_run) with no host synchronisation inside T.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <optional>
#include <vector>

#include "../../include/pf_ledh.h"
#include "pf_hooks.h"
#include "pf_host.h"
#include "pf_ledh_ekf.h"
#include "pf_ledh_kernels.h"
#include "pf_diag.h"
#include "pf_edh_kernels.h"
#include "pf_ledh_fused.h"
#include "pf_ledh_run_plan.h"
#include "pf_order.h"

namespace pf {
namespace ledh {

struct LOps {
  int nx, nz, tk, ok, psize;
  hipError_t (*setup)(const FlowParams&, double*, int, int, hipStream_t);  // (.., L, n_steps, ..)
  hipError_t (*flow_shared)(const FlowParams&, hipStream_t);
  hipError_t (*flow_wave)(const FlowParams&, int, hipStream_t);
  hipError_t (*normalise_chain)(const WParams&, hipStream_t);  // tile_max, exp_sum, normalise, decide
  hipError_t (*resample)(const WParams&, hipStream_t);
  hipError_t (*stats)(const WParams&, bool cov, hipStream_t);
  hipError_t (*init)(double*, double*, const double*, const double*, const double*, int64_t, int64_t, uint64_t,
                     uint32_t, hipStream_t);
  void (*prepare)();
  hipError_t (*ekf)(const double* Pm, const double* x0, const double* P0, const double* Qt, const double* Rt,
                    const double* Z, int64_t T, double* Ps, double* x_out, double* P_out, double* Xp, hipStream_t);
  // EDH (pf_edh_kernels.h): composed flow maps of n_steps time steps; the particle kernel (nonlinear h)
  hipError_t (*edh_setup)(const FlowParams&, double*, int, hipStream_t);
  hipError_t (*flow_edh)(const FlowParams&, hipStream_t);
  // the whole shared-path step in one cooperative launch (pf_ledh_fused.h); null for nonlinear h
  hipError_t (*fused)(const FusedParams&, hipStream_t);
  int (*fused_blocks_per_cu)();
  int fused_E;  // moment partial entries per workgroup
};

template <int NX, int NZ, int TK, int OK>
struct LL {
  // flow tables of n_steps time steps at once (P_k, z_k, table_k strided by the FlowParams strides)
  static hipError_t setup(const FlowParams& p, double* table, int L, int n_steps, hipStream_t s) {
    hipLaunchKernelGGL((k_setup<NX, NZ>), dim3(L, n_steps), dim3(SB), 0, s, p, table);
    const size_t lds = (size_t)L * (TLay<NX, NZ>::PJ) * sizeof(double);
    hipLaunchKernelGGL((k_compose<NX, NZ>), dim3(n_steps), dim3(SB), lds, s, table, p.lams, L, p.dlam,
                       p.table_stride);
    return hipGetLastError();
  }
  static hipError_t flow_shared(const FlowParams& p, hipStream_t s) {
    if constexpr (OK == PF_OBS_LINEAR) {
      const int64_t threads = p.N * Grp<NX>::GL;
      hipLaunchKernelGGL((k_flow_affine<NX, NZ, TK>), dim3((unsigned)((threads + TB - 1) / TB)), dim3(TB), 0, s, p);
      return hipGetLastError();
    } else {
      return hipErrorInvalidValue;
    }
  }
  static hipError_t flow_wave(const FlowParams& p, int grid, hipStream_t s) {
    if constexpr (OK == PF_OBS_ACOUSTIC) {
      // the acoustic h reads the positions only: the flow's algebra in their NX / 2 dimensions
      // (k_flow_wave_lr); PF_FLOW_LR=0 runs the observation-space kernel (A/B and the test that
      // compares the two), read per launch
      const char* lr_env = std::getenv("PF_FLOW_LR");
      const bool lr = !(lr_env && std::atoi(lr_env) == 0);
      if (lr && p.r_diag) {  // U = R^{-1/2} H8 by a diagonal scaling
        pf::lds_poison_hook(s);  // tests only (pf_hooks.h)
        FlowParams q = p;
        q.lr_force = pf::test_hook_int("PF_TEST_FLOW_LR_FORCE");  // tests only (pf_hooks.h)
        hipLaunchKernelGGL((k_flow_wave_lr<NX, NZ, TK>), dim3(grid), dim3(64), 0, s, q);
        return hipGetLastError();
      }
    }
    pf::lds_poison_hook(s);  // tests only (pf_hooks.h)
    hipLaunchKernelGGL((k_flow_wave<NX, NZ, TK, OK>), dim3(grid), dim3(64), 0, s, p);
    return hipGetLastError();
  }
  static hipError_t normalise_chain(const WParams& p, hipStream_t s) {
    if (p.N <= SMALL_N) {
      hipLaunchKernelGGL(k_weights_small, dim3(1), dim3(WB), (size_t)p.N * sizeof(double), s, p);
      return hipGetLastError();
    }
    hipLaunchKernelGGL(k_tile_max, dim3(p.G), dim3(TB), 0, s, p);
    hipLaunchKernelGGL(k_exp_sum, dim3(p.G), dim3(TB), 0, s, p);
    hipLaunchKernelGGL(k_normalise, dim3(p.G), dim3(TB), 0, s, p);
    hipLaunchKernelGGL(k_decide, dim3(1), dim3(TB), 0, s, p, 2);
    hipLaunchKernelGGL(k_cdf, dim3(p.G), dim3(TB), 0, s, p, 2);
    return hipGetLastError();
  }
  // ancestors + gather into x_out / w_out, or copy-through when the decision was "no resample"
  static hipError_t resample(const WParams& p, hipStream_t s) {
    const size_t lds = p.N <= GCAP ? (size_t)p.N * sizeof(double) : 0;
    hipLaunchKernelGGL((k_gather<NX>), dim3((unsigned)((p.N + TB - 1) / TB)), dim3(TB), lds, s, p);
    return hipGetLastError();
  }
  // posterior mean / cov (ledh.py:209, 217-224): one-pass shifted partials + final
  static hipError_t stats(const WParams& p, bool cov, hipStream_t s) {
    (void)cov;
    hipLaunchKernelGGL((k_mom_part<NX>), dim3(p.Gc), dim3(TB), 0, s, p);
    constexpr int NOUT = NX + NX * (NX + 1) / 2;
    hipLaunchKernelGGL((k_mom_final<NX>), dim3((NOUT + MF_E - 1) / MF_E), dim3(MF_E * MF_P), 0, s, p);
    return hipGetLastError();
  }
  static void prepare() {
    (void)hipFuncSetAttribute((const void*)k_gather<NX>, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(GCAP * sizeof(double)));
    (void)hipFuncSetAttribute((const void*)k_compose<NX, NZ>, hipFuncAttributeMaxDynamicSharedMemorySize, 120 * 1024);
    (void)hipFuncSetAttribute((const void*)k_weights_small, hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)(SMALL_N * sizeof(double)));
  }
  static hipError_t init(double* x, double* w, const double* mean0, const double* Lc, const double* eps, int64_t N,
                         int64_t Npad, uint64_t seed, uint32_t epoch, hipStream_t s) {
    hipLaunchKernelGGL((k_init<NX>), dim3((unsigned)((N + TB - 1) / TB)), dim3(TB), 0, s, x, w, mean0, Lc, eps, N,
                       Npad, seed, epoch);
    return hipGetLastError();
  }
  static hipError_t ekf(const double* Pm, const double* x0, const double* P0, const double* Qt, const double* Rt,
                        const double* Z, int64_t T, double* Ps, double* x_out, double* P_out, double* Xp,
                        hipStream_t s) {
    pf::lds_poison_hook(s);  // tests only (pf_hooks.h)
    hipLaunchKernelGGL((k_ekf_seq<NX, NZ, TK, OK>), dim3(1), dim3(ekf_block<NZ>()), 0, s, Pm, x0, P0, Qt, Rt, Z, T, Ps, x_out, P_out,
                       Xp);
    return hipGetLastError();
  }
  static hipError_t fused(const FusedParams& p, hipStream_t s) {
    if constexpr (OK == PF_OBS_LINEAR) {
      pf::lds_poison_hook(s);  // tests only (pf_hooks.h)
      hipLaunchKernelGGL((k_ledh_fused<NX, NZ, TK>), dim3(p.nbk), dim3(FusedBlk<NX>::FB), 0, s, p);
      return hipGetLastError();
    } else {
      return hipErrorInvalidValue;
    }
  }
  static int fused_blocks_per_cu() {
    if constexpr (OK == PF_OBS_LINEAR) {
      int nb = 0;
      if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void*)k_ledh_fused<NX, NZ, TK>, FusedBlk<NX>::FB,
                                                       0) !=
          hipSuccess)
        return 0;
      return nb;
    } else {
      return 0;
    }
  }
  static hipError_t edh_setup(const FlowParams& p, double* table, int n_steps, hipStream_t s) {
    hipLaunchKernelGGL((k_edh_setup<NX, NZ, TK, OK>), dim3(n_steps), dim3(SB), 0, s, p, table);
    return hipGetLastError();
  }
  static hipError_t flow_edh(const FlowParams& p, hipStream_t s) {
    if constexpr (OK == PF_OBS_LINEAR) {
      return flow_shared(p, s);  // eta_L = eta0 + d0 + D (H eta0): the LEDH affine kernel, theta = 0
    } else {
      hipLaunchKernelGGL((k_flow_edh<NX, NZ, TK, OK>), dim3((unsigned)((p.N + TB - 1) / TB)), dim3(TB), 0, s, p);
      return hipGetLastError();
    }
  }
  static LOps make() {
    LOps o;
    o.ekf = &ekf;
    o.edh_setup = &edh_setup;
    o.fused = (OK == PF_OBS_LINEAR) ? &fused : nullptr;
    o.fused_blocks_per_cu = &fused_blocks_per_cu;
    o.fused_E = Mom<NX>::E;
    o.flow_edh = &flow_edh;
    o.nx = NX; o.nz = NZ; o.tk = TK; o.ok = OK;
    o.psize = Lay<NX, NZ>::SIZE;
    static_assert(LedhLay(NX, NZ).SIZE == Lay<NX, NZ>::SIZE && LedhLay(NX, NZ).size(8) == TLay<NX, NZ>::size(8) &&
                      LedhLay(NX, NZ).table_size(8) >= (size_t)TLay<NX, NZ>::aff(8) + ELay<NX>::SIZE,
                  "the host's LedhLay(nx, nz) is this shape's Lay / TLay / ELay");
    o.setup = &setup;
    o.flow_shared = (OK == PF_OBS_LINEAR) ? &flow_shared : nullptr;
    o.flow_wave = &flow_wave;
    o.normalise_chain = &normalise_chain;
    o.resample = &resample;
    o.stats = &stats;
    o.init = &init;
    o.prepare = &prepare;
    return o;
  }
};

// compiled LEDH model shapes
static const std::vector<LOps>& lregistry() {
  static const std::vector<LOps> r = {
      LL<1, 1, PF_TRANS_LINEAR, PF_OBS_LINEAR>::make(),      // linear 1-D (test_ledh_flow_pf.py fixtures)
      LL<1, 1, PF_TRANS_LINEAR, PF_OBS_EXP_HALF>::make(),    // SV, h = beta exp(x/2)
      LL<2, 1, PF_TRANS_LINEAR, PF_OBS_LINEAR>::make(),      // 2-D linear test system
      LL<4, 9, PF_TRANS_LINEAR, PF_OBS_ACOUSTIC>::make(),    // one acoustic target, 3x3 sensors
      LL<4, 12, PF_TRANS_LINEAR, PF_OBS_ACOUSTIC>::make(),   // one acoustic target, 3x4 sensors
      LL<4, 25, PF_TRANS_LINEAR, PF_OBS_ACOUSTIC>::make(),   // one acoustic target, 5x5 sensors
      LL<16, 25, PF_TRANS_LINEAR, PF_OBS_ACOUSTIC>::make(),  // joint 4-target acoustic tracking
      LL<40, 10, PF_TRANS_L96, PF_OBS_LINEAR>::make(),       // Lorenz-96 d = 40 (BASELINE config 5)
  };
  return r;
}
static const LOps* find_lops(int nx, int nz, int tk, int ok) {
  for (const LOps& o : lregistry())
    if (o.nx == nx && o.nz == nz && o.tk == tk && o.ok == ok) return &o;
  return nullptr;
}

}  // namespace ledh
}  // namespace pf

using namespace pf::ledh;
using pf::GridOrderScope;
using pf::grid_order_forget;
using pf::DevBuf;
using pf::fail;
using pf::chol_lower;
using pf::spd_inverse;
using pf::is_diag;

struct pf_ledh_handle {
  const LOps* ops = nullptr;
  int nx = 0, nz = 0, tk = 0, ok = 0;
  int64_t N = 0, Npad = 0;
  int L = 1, G = 1, Gc = 1;
  double dlam = 1.0, ratio = 0.0;
  uint64_t seed = 0;
  int device = 0;
  bool shared = false;
  int algo = 0;   // 0 LEDH, 1 EDH (pf_edh_create)
  int integ = 0;  // EDH integrator (PF_EDH_RK4 / PF_EDH_EULER)
  int q_diag = 0, r_diag = 0;
  uint32_t epoch = 1;
  bool initialized = false;
  bool pending = false;  // the last step decided to resample
  pf::Stream stream;  // the streams before the buffers: destroyed after them
  pf::Stream side;    // tracker + flow tables, run ahead of the particle loop (pf_ledh_run_ekf)
  std::vector<double> lams;
  // device buffers
  DevBuf<double> x, x_alt, w, w_alt, lw;
  DevBuf<double> tmax, tsum, trec, cdf, stat, mean;
  DevBuf<double> mean_prev;  // shift of the one-pass moments (ping-pong with mean)
  DevBuf<double> mean3;      // third mean buffer of the fused run (shift of two steps back)
  DevBuf<double> cpart, Pm, Pk, z, u, vbuf;
  DevBuf<double> xbar;  // EDH: tracker past mean of the current step
  // fused shared-path step (pf_ledh_fused.h): grid geometry, barrier words, partials
  int fused_nbk = 0, fused_ppb = 0;
  unsigned long long fphase = 0;
  DevBuf<unsigned long long> fpart, fcpart;
  int fcp = 0;  // which half of fcpart the last fused step's P4 wrote
  DevBuf<int32_t> fanc;  // [N] ancestors of the slots between fused steps
  // run_impl's device buffers (tracker covariances, observations, outputs, flow tables), one
  // allocation kept across runs: a run allocates only when it needs more than the last one
  DevBuf<char> arena;
  size_t arena_bytes = 0;
  DevBuf<unsigned int> ferr;
  DevBuf<double> table, d_lams, diagS, out, unif, Lc;
  // replayed draws for the next run (pf_ledh_set_run_replay): noise [T][N][nx], U [T]
  DevBuf<double> rp_noise, rp_unif;
  int64_t rp_T = 0;
  ~pf_ledh_handle() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    if (side) (void)hipStreamSynchronize(side);
    if (stream) grid_order_forget(device, stream);
  }
};

namespace {

FlowParams flow_params(pf_ledh_handle* h, const double* Pk, const double* z, const double* u, int noise,
                       const double* v, double* diagS) {
  FlowParams p;
  p.x_in = h->x;
  p.x_out = h->x_alt;
  p.w_in = h->w;
  p.lw = h->lw;
  p.Pm = h->Pm;
  p.Pk = Pk;
  p.z = z;
  p.u = u;
  p.v_host = v;
  p.table = h->table;
  p.pk_stride = p.z_stride = p.table_stride = 0;
  p.lams = h->d_lams;
  p.diagS = diagS;
  p.N = h->N;
  p.Npad = h->Npad;
  p.L = h->L;
  p.dlam = h->dlam;
  p.noise = noise;
  p.seed = h->seed;
  p.epoch = h->epoch;
  p.q_diag = h->q_diag;
  p.r_diag = h->r_diag;
  p.xbar = nullptr;
  p.xbar_stride = p.u_stride = 0;
  p.integ = h->integ;
  return p;
}

WParams w_params(pf_ledh_handle* h) {
  WParams p;
  p.x_in = h->x;
  p.x_out = h->x_alt;
  p.lw = h->lw;
  p.w = h->w;
  p.w_out = h->w_alt;
  p.tmax = h->tmax;
  p.tsum = h->tsum;
  p.trec = h->trec;
  p.cdf = h->cdf;
  p.stat = h->stat;
  p.mean = h->mean;
  p.shift = h->mean_prev;
  p.cpart = h->cpart;
  p.o_mean = p.o_cov = p.o_ess = nullptr;
  p.o_flag = nullptr;
  p.unif = nullptr;
  p.N = h->N;
  p.Npad = h->Npad;
  p.G = h->G;
  p.Gc = h->Gc;
  p.ratio = h->ratio;
  p.seed = h->seed;
  p.epoch = 0;
  p.uniform = 0;
  return p;
}

// flow + weights + decision of one step (ledh.py:104-203), all enqueued on h->stream
pf_status enqueue_flow(pf_ledh_handle* h, const double* Pk, const double* z, const double* u, int noise,
                       const double* v, double* diagS, double* o_ess, int32_t* o_flag,
                       const double* pre_table = nullptr, const double* xbar = nullptr) {
  const uint32_t ep_noise = ++h->epoch;
  FlowParams fp = flow_params(h, Pk, z, u, noise, v, diagS);
  fp.epoch = ep_noise;
  if (h->algo == 1) {  // EDH: one composed affine map per step (pf_edh_kernels.h)
    if (pre_table) {
      fp.table = pre_table;
    } else {
      fp.xbar = xbar;
      PF_HIPCHK(h->ops->edh_setup(fp, h->table, 1, h->stream));
    }
    PF_HIPCHK(h->ops->flow_edh(fp, h->stream));
  } else if (h->shared) {
    if (pre_table) fp.table = pre_table;  // built for the whole run up front (pf_ledh_run)
    else PF_HIPCHK(h->ops->setup(fp, h->table, h->L, 1, h->stream));
    PF_HIPCHK(h->ops->flow_shared(fp, h->stream));
  } else {
    int grid = (int)std::min<int64_t>(h->N, 256 * 16);
    PF_HIPCHK(h->ops->flow_wave(fp, grid, h->stream));
  }
  std::swap(h->x, h->x_alt);  // the flowed particles are current
  WParams wp = w_params(h);
  wp.o_ess = o_ess;
  wp.o_flag = o_flag;
  PF_HIPCHK(h->ops->normalise_chain(wp, h->stream));
  return PF_OK;
}

// resample (flag on the device) with the uniform at U (device; null: Philox); the result is current
pf_status enqueue_resample(pf_ledh_handle* h, const double* U) {
  WParams wp = w_params(h);
  wp.unif = U;
  wp.epoch = ++h->epoch;
  PF_HIPCHK(h->ops->resample(wp, h->stream));
  std::swap(h->x, h->x_alt);
  std::swap(h->w, h->w_alt);
  return PF_OK;
}

// posterior moments of the current state into o_mean / o_cov (device; null: not stored)
pf_status enqueue_moments(pf_ledh_handle* h, double* o_mean, double* o_cov, bool uniform) {
  WParams sp = w_params(h);
  sp.uniform = uniform ? 1 : 0;
  sp.o_mean = o_mean;
  sp.o_cov = o_cov;
  PF_HIPCHK(h->ops->stats(sp, true, h->stream));
  std::swap(h->mean, h->mean_prev);  // the new mean is the next moments' shift
  return PF_OK;
}

// resample + posterior moments of one step of the kernel chain
pf_status enqueue_finish(pf_ledh_handle* h, const double* U, double* o_mean, double* o_cov) {
  if (pf_status st = enqueue_resample(h, U); st != PF_OK) return st;
  return enqueue_moments(h, o_mean, o_cov, false);
}

// the moments of the current state, waited for and copied to the host: mean (now in mean_prev) and
// cov (staged in out[nx : nx + nx*nx)), each optional
pf_status moments_to_host(pf_ledh_handle* h, bool uniform, double* mean, double* cov) {
  const int nx = h->nx;
  if (pf_status st = enqueue_moments(h, nullptr, h->out + nx, uniform); st != PF_OK) return st;
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  if (mean) PF_HIPCHK(hipMemcpy(mean, h->mean_prev, nx * 8, hipMemcpyDeviceToHost));
  if (cov) PF_HIPCHK(hipMemcpy(cov, h->out + nx, (size_t)nx * nx * 8, hipMemcpyDeviceToHost));
  return PF_OK;
}

// particles between the caller's [N][nx] rows and the device's [nx][Npad] columns
void aos_to_soa(const pf_ledh_handle* h, const double* aos, std::vector<double>& soa) {
  soa.assign((size_t)h->nx * h->Npad, 0.0);
  for (int64_t i = 0; i < h->N; ++i)
    for (int d = 0; d < h->nx; ++d) soa[(size_t)d * h->Npad + i] = aos[i * h->nx + d];
}
void soa_to_aos(const pf_ledh_handle* h, const std::vector<double>& soa, double* aos) {
  for (int64_t i = 0; i < h->N; ++i)
    for (int d = 0; d < h->nx; ++d) aos[i * h->nx + d] = soa[(size_t)d * h->Npad + i];
}

pf_status sym_upload(pf_ledh_handle* h, const double* P, double* dst) {
  const int n = h->nx;
  std::vector<double> S((size_t)n * n);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) S[i * n + j] = 0.5 * (P[i * n + j] + P[j * n + i]);  // ledh.py:106
  PF_HIPCHK(hipMemcpyAsync(dst, S.data(), S.size() * sizeof(double), hipMemcpyHostToDevice, h->stream));
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  return PF_OK;
}

}  // namespace

extern "C" {

int32_t pf_ledh_model_supported(int32_t nx, int32_t nz, int32_t tk, int32_t ok) {
  return find_lops(nx, nz, tk, ok) != nullptr;
}

}  // extern "C"

// LEDHFlowPF.__init__ (ledh.py:63-81) / EDHFlowPF.__init__ (edh.py:138-171): algo 0 LEDH, 1 EDH
static pf_status create_impl(const pf_model_desc* m, const pf_ledh_opts* o, int algo, int integ,
                             pf_ledh_handle** out) {
  if (!m || !o || !out) return fail(PF_E_ARG, "null argument");
  *out = nullptr;
  if (o->n_particles <= 0) return fail(PF_E_ARG, "n_particles must be positive");
  if (o->n_particles > (int64_t)LT * MAXT) return fail(PF_E_ARG, "n_particles too large (max 1048576)");
  const LOps* ops = find_lops(m->nx, m->nz, m->trans_kind, m->obs_kind);
  if (!ops)
    return fail(PF_E_UNSUPPORTED, "LEDH model (nx=" + std::to_string(m->nx) + ", nz=" + std::to_string(m->nz) +
                                       ", g=" + std::to_string(m->trans_kind) + ", h=" + std::to_string(m->obs_kind) +
                                       ") is not compiled into libpf_hip");
  const int nx = m->nx, nz = m->nz;
  std::vector<double> P((size_t)ops->psize, 0.0);
  const LedhLay lay(nx, nz);
  if (m->trans_kind == PF_TRANS_LINEAR) {
    if (m->n_trans_params < (int64_t)nx * nx || !m->trans_params) return fail(PF_E_ARG, "LINEAR g needs A[nx*nx]");
    for (int i = 0; i < nx * nx; ++i) P[lay.A + i] = m->trans_params[i];
  } else if (m->trans_kind == PF_TRANS_L96) {
    if (m->n_trans_params < 2 || !m->trans_params) return fail(PF_E_ARG, "L96 g needs {F, dt}");
    P[lay.EX] = m->trans_params[0];
    P[lay.EX + 1] = m->trans_params[1];
  }
  if (m->obs_kind == PF_OBS_LINEAR) {
    if (m->n_obs_params < (int64_t)nz * nx + nz || !m->obs_params) return fail(PF_E_ARG, "LINEAR h needs H, c");
    for (int i = 0; i < nz * nx; ++i) P[lay.H + i] = m->obs_params[i];
    for (int i = 0; i < nz; ++i) P[lay.C + i] = m->obs_params[nz * nx + i];
  } else if (m->obs_kind == PF_OBS_EXP_HALF) {
    if (m->n_obs_params < nz || !m->obs_params) return fail(PF_E_ARG, "EXP_HALF h needs beta[nz]");
    for (int i = 0; i < nz; ++i) P[lay.C + i] = m->obs_params[i];
  } else if (m->obs_kind == PF_OBS_ACOUSTIC) {
    if (m->n_obs_params < 2 + 2 * nz || !m->obs_params) return fail(PF_E_ARG, "ACOUSTIC h needs psi, d0, sx, sy");
    for (int i = 0; i < 2 + 2 * nz; ++i) P[lay.AC + i] = m->obs_params[i];
  }
  if (!m->Q || !m->R) return fail(PF_E_ARG, "Q and R are required");
  std::vector<double> Lq, Qi, Ri;
  if (!chol_lower(m->Q, nx, 0.0, Lq) && !chol_lower(m->Q, nx, 1e-10, Lq))
    return fail(PF_E_NOT_PD, "Matrix is not positive definite (Q)");
  if (!spd_inverse(m->Q, nx, Qi)) return fail(PF_E_NOT_PD, "Matrix is not positive definite (Q)");
  if (!spd_inverse(m->R, nz, Ri)) return fail(PF_E_NOT_PD, "Matrix is not positive definite (R)");
  for (int i = 0; i < nx * nx; ++i) {
    P[lay.LQ + i] = Lq[i];
    P[lay.QI + i] = Qi[i];
  }
  for (int i = 0; i < nz * nz; ++i) {
    P[lay.R + i] = m->R[i];
    P[lay.RI + i] = Ri[i];
  }
  PF_HIPCHK(hipSetDevice(o->device));
  std::unique_ptr<pf_ledh_handle> hp(new pf_ledh_handle());
  pf_ledh_handle* h = hp.get();
  h->ops = ops;
  h->nx = nx; h->nz = nz; h->tk = m->trans_kind; h->ok = m->obs_kind;
  h->N = o->n_particles;
  h->Npad = (h->N + 3) / 4 * 4;
  h->L = std::max(1, (int)o->n_lambda);                   // ledh.py:132
  h->algo = algo;
  h->integ = integ;
  // the shared-Jacobian path stages its whole flow table in LDS; past that size (many lambda
  // steps) a linear h takes the per-particle flow instead (the same flow, particle by particle)
  const bool table_fits = (size_t)h->L * (size_t)lay.TPJ * 8 <= 120 * 1024;
  h->dlam = 1.0 / (double)h->L;                           // ledh.py:133
  double lam = 0.0;
  for (int j = 0; j < h->L; ++j) {                        // ledh.py:134-137
    lam = std::min(1.0, lam + h->dlam);
    h->lams.push_back(lam);
  }
  h->ratio = o->resample_ess_ratio;
  h->seed = o->seed;
  h->device = o->device;
  h->shared = ops->flow_shared && o->flow_mode == PF_LEDH_FLOW_AUTO && (algo != 0 || table_fits);
  h->q_diag = is_diag(Qi.data(), nx);
  h->r_diag = is_diag(Ri.data(), nz);
  h->G = (int)((h->N + LT - 1) / LT);
  h->Gc = (int)((h->N + CT * CTS - 1) / (CT * CTS));
  PF_HIPCHK(hipStreamCreateWithFlags(h->stream.out(), hipStreamNonBlocking));
  PF_HIPCHK(hipStreamCreateWithFlags(h->side.out(), hipStreamNonBlocking));
  const size_t xn = (size_t)nx * h->Npad, xb = xn * sizeof(double), nn = (size_t)h->N;
  const int NP = nx * (nx + 1) / 2;
  struct A { DevBuf<double>* p; size_t n; };  // doubles
  A allocs[] = {{&h->x, xn}, {&h->x_alt, xn}, {&h->w, nn}, {&h->w_alt, nn}, {&h->lw, nn}, {&h->cdf, nn},
                {&h->tmax, (size_t)h->G}, {&h->tsum, (size_t)h->G}, {&h->trec, (size_t)h->G * (2 + nx)},
                {&h->stat, 8}, {&h->mean, (size_t)nx}, {&h->mean_prev, (size_t)nx}, {&h->mean3, (size_t)nx},
                {&h->cpart, (size_t)h->Gc * (1 + nx + NP)},
                {&h->Pm, P.size()}, {&h->Pk, (size_t)nx * nx}, {&h->z, (size_t)nz},
                {&h->u, (size_t)nx}, {&h->table, lay.table_size(h->L)}, {&h->d_lams, (size_t)h->L},
                {&h->diagS, (size_t)h->L * nz * nz}, {&h->out, (size_t)(nx + nx * nx + 2)},
                {&h->unif, 1}, {&h->Lc, (size_t)nx * nx}};
  for (auto& a : allocs) PF_HIPCHK(a.p->alloc(a.n));
  PF_HIPCHK(hipMemset(h->x, 0, xb));
  PF_HIPCHK(hipMemset(h->x_alt, 0, xb));
  PF_HIPCHK(hipMemset(h->mean, 0, (size_t)nx * 8));
  PF_HIPCHK(hipMemset(h->mean_prev, 0, (size_t)nx * 8));
  ops->prepare();
  PF_HIPCHK(hipMemcpy(h->Pm, P.data(), P.size() * 8, hipMemcpyHostToDevice));
  PF_HIPCHK(hipMemcpy(h->d_lams, h->lams.data(), h->lams.size() * 8, hipMemcpyHostToDevice));
  if (algo == 1) PF_HIPCHK(h->xbar.alloc((size_t)nx));
  // fused step geometry: <= one workgroup per CU, all co-resident (PF_LEDH_FUSED=0 disables)
  {
    const char* env = std::getenv("PF_LEDH_FUSED");
    const bool want = ops->fused && (h->shared || algo == 1) && !(env && env[0] == '0');
    int cus = 0;
    PF_HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, h->device));
    const int per_cu = want ? ops->fused_blocks_per_cu() : 0;
    int64_t ppb = 64;
    while ((h->N + ppb - 1) / ppb > FMAX && ppb < FPPB) ppb += 64;
    const int64_t nbk = (h->N + ppb - 1) / ppb;
    if (want && nbk <= FMAX && nbk <= (int64_t)per_cu * cus) {
      h->fused_nbk = (int)nbk;
      h->fused_ppb = (int)ppb;
      PF_HIPCHK(h->fpart.alloc(8 * FMAX));
      PF_HIPCHK(h->fcpart.alloc(2 * (size_t)FMAX * ops->fused_E));
      PF_HIPCHK(h->fanc.alloc((size_t)h->N));
      PF_HIPCHK(h->ferr.alloc(2));
      PF_HIPCHK(hipMemset(h->fpart, 0, 8 * FMAX * 8));  // tag 0: never a launch's (tags start at 1)
      PF_HIPCHK(hipMemset(h->ferr, 0, 8));
    }
  }
  *out = hp.release();
  return PF_OK;
}

extern "C" {

pf_status pf_ledh_create(const pf_model_desc* m, const pf_ledh_opts* o, pf_ledh_handle** out) try {
  return create_impl(m, o, 0, 0, out);
} catch (...) { return pf::on_exception("pf_ledh_create"); }

pf_status pf_edh_create(const pf_model_desc* m, const pf_edh_opts* o, pf_ledh_handle** out) try {
  if (!o) return fail(PF_E_ARG, "null argument");
  if (o->integrator != PF_EDH_RK4 && o->integrator != PF_EDH_EULER) return fail(PF_E_ARG, "bad EDH integrator");
  pf_ledh_opts lo;
  lo.n_particles = o->n_particles;
  lo.n_lambda = o->n_lambda;
  lo.resample_ess_ratio = o->resample_ess_ratio;
  lo.seed = o->seed;
  lo.device = o->device;
  lo.flow_mode = PF_LEDH_FLOW_AUTO;
  return create_impl(m, &lo, 1, o->integrator, out);
} catch (...) { return pf::on_exception("pf_edh_create"); }

int32_t pf_edh_is_edh(pf_ledh_handle* h) { return (h && h->algo == 1) ? 1 : 0; }

void pf_ledh_destroy(pf_ledh_handle* h) { delete h; }

pf_status pf_ledh_init(pf_ledh_handle* h, const double* mean0, const double* cov0, const double* eps,
                       double* mean_out, double* cov_out) try {
  if (!h || !mean0 || !cov0) return fail(PF_E_ARG, "null argument");
  PF_HIPCHK(hipSetDevice(h->device));
  const int nx = h->nx;
  std::vector<double> L;
  if (!eps && !chol_lower(cov0, nx, 0.0, L) && !chol_lower(cov0, nx, 1e-10, L))
    return fail(PF_E_NOT_PD, "Matrix is not positive definite (cov0)");
  if (eps) L.assign((size_t)nx * nx, 0.0);
  double* dm = h->out;  // staging: mean0 in out[0..nx)
  double* deps = nullptr;
  PF_HIPCHK(hipMemcpyAsync(dm, mean0, nx * 8, hipMemcpyHostToDevice, h->stream));
  PF_HIPCHK(hipMemcpyAsync(h->Lc, L.data(), L.size() * 8, hipMemcpyHostToDevice, h->stream));
  if (eps) {
    if (!h->vbuf) PF_HIPCHK(h->vbuf.alloc((size_t)h->N * nx));
    PF_HIPCHK(hipMemcpyAsync(h->vbuf, eps, (size_t)h->N * nx * 8, hipMemcpyHostToDevice, h->stream));
    deps = h->vbuf;
  }
  h->epoch = 1;
  PF_HIPCHK(h->ops->init(h->x, h->w, dm, h->Lc, deps, h->N, h->Npad, h->seed, h->epoch, h->stream));
  // _weighted_stats of the initial set (ledh.py:90), shifted by zero as on a new handle: whatever mean
  // an earlier run left in mean_prev would round the moments differently, and a re-initialised handle
  // must repeat a new one to the bit
  PF_HIPCHK(hipMemsetAsync(h->mean_prev, 0, nx * 8, h->stream));
  if (pf_status st = moments_to_host(h, true, mean_out, cov_out); st != PF_OK) return st;
  h->initialized = true;
  h->pending = false;
  return PF_OK;
} catch (...) { return pf::on_exception("pf_ledh_init"); }

static pf_status step_impl(pf_ledh_handle* h, const double* P, const double* xbar, const double* z, const double* u,
                           int32_t noise, const double* v, pf_ledh_info* info, double* cond_S);

pf_status pf_ledh_step(pf_ledh_handle* h, const double* P, const double* z, const double* u, int32_t noise,
                       const double* v, pf_ledh_info* info, double* cond_S) try {
  if (h && h->algo == 1) return fail(PF_E_ARG, "EDH handle: use pf_edh_step (it needs the tracker's past mean)");
  return step_impl(h, P, nullptr, z, u, noise, v, info, cond_S);
} catch (...) { return pf::on_exception("pf_ledh_step"); }

pf_status pf_edh_step(pf_ledh_handle* h, const double* P, const double* xbar, const double* z, const double* u,
                      int32_t noise, const double* v, pf_ledh_info* info, double* cond_S) try {
  if (h && h->algo != 1) return fail(PF_E_ARG, "pf_edh_step needs a handle from pf_edh_create");
  if (!xbar) return fail(PF_E_ARG, "null argument");
  return step_impl(h, P, xbar, z, u, noise, v, info, cond_S);
} catch (...) { return pf::on_exception("pf_edh_step"); }

}  // extern "C"

static pf_status step_impl(pf_ledh_handle* h, const double* P, const double* xbar, const double* z, const double* u,
                           int32_t noise, const double* v, pf_ledh_info* info, double* cond_S) {
  if (!h || !P || !z) return fail(PF_E_ARG, "null argument");
  if (!h->initialized) return fail(PF_E_NOT_INITIALIZED, "Filter not initialized.");
  if (noise == PF_NOISE_HOST && !v) return fail(PF_E_ARG, "PF_NOISE_HOST needs v");
  if (noise < PF_NOISE_NONE || noise > PF_NOISE_DEVICE) return fail(PF_E_ARG, "bad noise mode");
  PF_HIPCHK(hipSetDevice(h->device));
  if (sym_upload(h, P, h->Pk) != PF_OK) return PF_E_HIP;
  PF_HIPCHK(hipMemcpyAsync(h->z, z, h->nz * 8, hipMemcpyHostToDevice, h->stream));
  if (u) PF_HIPCHK(hipMemcpyAsync(h->u, u, h->nx * 8, hipMemcpyHostToDevice, h->stream));
  if (xbar) PF_HIPCHK(hipMemcpyAsync(h->xbar, xbar, h->nx * 8, hipMemcpyHostToDevice, h->stream));
  if (noise == PF_NOISE_HOST) {
    if (!h->vbuf) PF_HIPCHK(h->vbuf.alloc((size_t)h->N * h->nx));
    PF_HIPCHK(hipMemcpyAsync(h->vbuf, v, (size_t)h->N * h->nx * 8, hipMemcpyHostToDevice, h->stream));
  }
  pf_status st = enqueue_flow(h, h->Pk, h->z, u ? h->u : nullptr, noise, noise == PF_NOISE_HOST ? h->vbuf : nullptr,
                              cond_S ? h->diagS : nullptr, nullptr, nullptr, nullptr, xbar ? h->xbar : nullptr);
  if (st != PF_OK) return st;
  double stat[3];
  PF_HIPCHK(hipMemcpyAsync(stat, h->stat, 3 * 8, hipMemcpyDeviceToHost, h->stream));
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  if (cond_S) PF_HIPCHK(hipMemcpy(cond_S, h->diagS, (size_t)h->L * h->nz * h->nz * 8, hipMemcpyDeviceToHost));
  h->pending = stat[1] != 0.0;
  if (info) {
    info->ess = stat[0];
    info->resample = h->pending ? 1 : 0;
    info->_pad = 0;
  }
  return PF_OK;
}

extern "C" {

pf_status pf_ledh_finish(pf_ledh_handle* h, const double* U, double* mean, double* cov) try {
  if (!h) return fail(PF_E_ARG, "null argument");
  if (!h->initialized) return fail(PF_E_NOT_INITIALIZED, "Filter not initialized.");
  PF_HIPCHK(hipSetDevice(h->device));
  if (h->pending) {
    if (U) PF_HIPCHK(hipMemcpyAsync(h->unif, U, 8, hipMemcpyHostToDevice, h->stream));
    if (pf_status st = enqueue_resample(h, U ? h->unif : nullptr); st != PF_OK) return st;
    h->pending = false;
  }
  return moments_to_host(h, false, mean, cov);
} catch (...) { return pf::on_exception("pf_ledh_finish"); }

pf_status pf_ledh_get_particles(pf_ledh_handle* h, double* particles) try {
  if (!h || !particles) return fail(PF_E_ARG, "null argument");
  if (!h->initialized) return fail(PF_E_NOT_INITIALIZED, "Filter not initialized.");
  PF_HIPCHK(hipSetDevice(h->device));
  std::vector<double> soa((size_t)h->nx * h->Npad);
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  PF_HIPCHK(hipMemcpy(soa.data(), h->x, soa.size() * 8, hipMemcpyDeviceToHost));
  soa_to_aos(h, soa, particles);
  return PF_OK;
} catch (...) { return pf::on_exception("pf_ledh_get_particles"); }

pf_status pf_ledh_get_weights(pf_ledh_handle* h, double* weights) try {
  if (!h || !weights) return fail(PF_E_ARG, "null argument");
  if (!h->initialized) return fail(PF_E_NOT_INITIALIZED, "Filter not initialized.");
  PF_HIPCHK(hipSetDevice(h->device));
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  PF_HIPCHK(hipMemcpy(weights, h->w, (size_t)h->N * 8, hipMemcpyDeviceToHost));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_ledh_get_weights"); }

// diag:61-91 on the device-resident state (include/pf_diag.h)
pf_status pf_ledh_diagnostics(pf_ledh_handle* h, double tol, pf_diagnostics* out) try {
  if (!h || !out) return fail(PF_E_ARG, "null argument");
  if (!h->initialized) return fail(PF_E_NOT_INITIALIZED, "Filter not initialized.");
  PF_HIPCHK(hipSetDevice(h->device));
  pf::diag::DiagSrc s{};
  s.N = h->N;
  s.Npad = h->Npad;
  s.nx = h->nx;
  s.w = h->w;
  s.x = h->x;
  s.real_is_double = 1;
  s.tol = tol;
  s.spread = NAN;
  return pf::diag::compute(s, h->stream, out);
} catch (...) { return pf::on_exception("pf_ledh_diagnostics"); }

pf_status pf_ledh_set_state(pf_ledh_handle* h, const double* particles, const double* weights) try {
  if (!h || !particles || !weights) return fail(PF_E_ARG, "null argument");
  PF_HIPCHK(hipSetDevice(h->device));
  std::vector<double> soa;
  aos_to_soa(h, particles, soa);
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  PF_HIPCHK(hipMemcpy(h->x, soa.data(), soa.size() * 8, hipMemcpyHostToDevice));
  PF_HIPCHK(hipMemcpy(h->w, weights, (size_t)h->N * 8, hipMemcpyHostToDevice));
  h->initialized = true;
  h->pending = false;
  return PF_OK;
} catch (...) { return pf::on_exception("pf_ledh_set_state"); }

}  // extern "C"

namespace {

// Device EKF spec: host arrays (x0, P0, Qt, Rt) or all null.
struct EkfSpec {
  const double *x0, *P0, *Qt, *Rt;
  double *x_final, *P_final;
};

// The T loop (pf_ledh_run / pf_edh_run / pf_ledh_run_ekf): tracker covariances from the host (Ps) or
// from the device EKF, all flow tables built ahead of the steps that use them, then flow -> weights ->
// resample -> moments per step.  EDH handles also take the tracker's past means Xb [T][nx] (host) or
// get them from the device EKF.  A run is the stages below in the order run_impl calls them; its
// bookkeeping (arena layout, EKF slots, chunk schedule, mean ring) is pf_ledh_run_plan.h.

// One run's arguments, what follows from them, and its buffers in the handle's arena.
struct Run {
  pf_ledh_handle* h;
  const double *Ps, *Xb;
  const EkfSpec* ekf;
  const double *Z, *U;
  int64_t T;
  int32_t noise;
  int nx, nz;
  bool edh, replay, tabled;
  size_t tsz;     // doubles of one step's flow table
  EkfSlots slot;  // of dE
  double *dP = nullptr, *dZ = nullptr, *dU = nullptr, *dm = nullptr, *dc = nullptr, *de = nullptr;
  int32_t* df = nullptr;
  double *dE = nullptr, *dX = nullptr, *dTab = nullptr;
  std::vector<double> sym;       // the symmetrised Ps, alive until the upload has run
  std::vector<int64_t> cbeg;     // device tracker: first step of each chunk
  pf::Event uploaded;            // the EKF inputs are on the device
  std::vector<pf::Event> ready;  // chunk k's covariances, past means and tables are on the device

  Run(pf_ledh_handle* h_, const double* Ps_, const double* Xb_, const EkfSpec* ekf_, const double* Z_,
      const double* U_, int64_t T_, int32_t noise_)
      : h(h_), Ps(Ps_), Xb(Xb_), ekf(ekf_), Z(Z_), U(U_), T(T_), noise(noise_), nx(h_->nx), nz(h_->nz),
        edh(h_->algo == 1), replay(noise_ == PF_NOISE_HOST), tabled(h_->shared || h_->algo == 1),
        tsz(LedhLay(h_->nx, h_->nz).table_size(h_->L)), slot(h_->nx, h_->nz) {}

  bool fused() const { return h->fused_nbk > 0 && dTab; }  // the whole step in one launch (pf_ledh_fused.h)
  // step t's inputs and outputs
  const double* u_at(int64_t t) const { return dU ? dU + t * nx : nullptr; }
  const double* noise_at(int64_t t) const { return replay ? h->rp_noise + t * h->N * nx : nullptr; }
  const double* unif_at(int64_t t) const { return replay ? h->rp_unif + t : nullptr; }
  double* mean_at(int64_t t) const { return dm + t * nx; }
  double* cov_at(int64_t t) const { return dc + t * nx * nx; }
};

// stage: the readiness checks (no state is touched)
pf_status run_ready(pf_ledh_handle* h, const double* Ps, const double* Xb, const EkfSpec* ekf, const double* Z,
                    int64_t T, int32_t noise) {
  if (!h || !Z || (!Ps && !ekf)) return fail(PF_E_ARG, "null argument");
  if (h->algo == 1 && !ekf && !Xb) return fail(PF_E_ARG, "EDH run needs the tracker's past means");
  if (!h->initialized) return fail(PF_E_NOT_INITIALIZED, "Filter not initialized.");
  if (noise == PF_NOISE_HOST && h->rp_T != T)
    return fail(PF_E_ARG, "run: PF_NOISE_HOST needs pf_ledh_set_run_replay with the run's T");
  if (noise < PF_NOISE_NONE || noise > PF_NOISE_DEVICE) return fail(PF_E_ARG, "run: bad noise mode");
  return PF_OK;
}

// stage: the run's buffers in the handle's arena.  The arena only grows: a run allocates when it
// needs more than the last one, after both streams have let go of the old allocation.
pf_status run_carve(Run& r) {
  pf_ledh_handle* h = r.h;
  const RunArena a = run_arena(r.nx, r.nz, r.T, r.tsz, r.U != nullptr, r.ekf != nullptr, r.edh, r.tabled);
  if (a.total > h->arena_bytes) {
    if (h->arena) {
      PF_HIPCHK(hipStreamSynchronize(h->stream));
      PF_HIPCHK(hipStreamSynchronize(h->side));
    }
    h->arena_bytes = 0;
    PF_HIPCHK(h->arena.alloc(a.total));
    h->arena_bytes = a.total;
  }
  char* base = h->arena;
  r.dP = a.at<double>(base, RUN_P);
  r.dZ = a.at<double>(base, RUN_Z);
  r.dU = a.at<double>(base, RUN_U);
  r.dm = a.at<double>(base, RUN_MEANS);
  r.dc = a.at<double>(base, RUN_COVS);
  r.de = a.at<double>(base, RUN_ESS);
  r.df = a.at<int32_t>(base, RUN_FLAGS);
  r.dE = a.at<double>(base, RUN_EKF);
  r.dX = a.at<double>(base, RUN_XBAR);
  r.dTab = a.at<double>(base, RUN_TABLES);
  return PF_OK;
}

// stage: the host's inputs onto the device (the device tracker's own are run_tracker_ahead's)
pf_status run_upload(Run& r) {
  const int nx = r.nx, nz = r.nz;
  const int64_t T = r.T;
  hipStream_t s = r.h->stream;
  if (r.Ps) {
    r.sym.resize((size_t)T * nx * nx);
    for (int64_t t = 0; t < T; ++t)
      for (int i = 0; i < nx; ++i)
        for (int j = 0; j < nx; ++j)
          r.sym[(t * nx + i) * nx + j] = 0.5 * (r.Ps[(t * nx + i) * nx + j] + r.Ps[(t * nx + j) * nx + i]);  // ledh.py:106
    PF_HIPCHK(hipMemcpyAsync(r.dP, r.sym.data(), r.sym.size() * 8, hipMemcpyHostToDevice, s));
  }
  PF_HIPCHK(hipMemcpyAsync(r.dZ, r.Z, (size_t)T * nz * 8, hipMemcpyHostToDevice, s));
  if (r.U) PF_HIPCHK(hipMemcpyAsync(r.dU, r.U, (size_t)T * nx * 8, hipMemcpyHostToDevice, s));
  if (r.edh && !r.ekf) PF_HIPCHK(hipMemcpyAsync(r.dX, r.Xb, (size_t)T * nx * 8, hipMemcpyHostToDevice, s));
  return PF_OK;
}

// flow tables of steps [c0, c0 + n) on stream s (they depend on (P_k, z_k) only, not on the particles)
pf_status run_tables(const Run& r, int64_t c0, int64_t n, hipStream_t s) {
  if (!r.tabled) return PF_OK;
  pf_ledh_handle* h = r.h;
  const int nx = r.nx, nz = r.nz;
  FlowParams fp = flow_params(h, r.dP + c0 * nx * nx, r.dZ + c0 * nz, nullptr, r.noise, nullptr, nullptr);
  fp.pk_stride = (int64_t)nx * nx;
  fp.z_stride = nz;
  fp.table_stride = (int64_t)r.tsz;
  if (r.edh) {
    fp.xbar = r.dX + c0 * nx;
    fp.xbar_stride = nx;
    fp.u = r.u_at(c0);
    fp.u_stride = nx;
    PF_HIPCHK(h->ops->edh_setup(fp, r.dTab + c0 * r.tsz, (int)n, s));
  } else {
    PF_HIPCHK(h->ops->setup(fp, r.dTab + c0 * r.tsz, h->L, (int)n, s));
  }
  return PF_OK;
}

// stage, host tracker: every table up front on the particle stream
pf_status run_tables_upfront(const Run& r) {
  for (int64_t c0 = 0; c0 < r.T; c0 += 65535)  // grid.y <= 65535 steps per launch
    if (pf_status st = run_tables(r, c0, std::min<int64_t>(65535, r.T - c0), r.h->stream); st != PF_OK) return st;
  return PF_OK;
}

// stage, device tracker: the EKF and the tables run on the side stream in chunks of steps
// (run_chunk_starts), ahead of the particle loop, which waits for each chunk's event (the tracker
// never needs the particles)
pf_status run_tracker_ahead(Run& r) {
  pf_ledh_handle* h = r.h;
  const int nx = r.nx, nz = r.nz;
  const EkfSpec& e = *r.ekf;
  double *x0 = r.dE + r.slot.x0, *P0 = r.dE + r.slot.P0, *Qt = r.dE + r.slot.Qt, *Rt = r.dE + r.slot.Rt;
  double *xf = r.dE + r.slot.x_final, *Pf = r.dE + r.slot.P_final;
  PF_HIPCHK(hipMemcpyAsync(x0, e.x0, nx * 8, hipMemcpyHostToDevice, h->stream));
  PF_HIPCHK(hipMemcpyAsync(P0, e.P0, (size_t)nx * nx * 8, hipMemcpyHostToDevice, h->stream));
  PF_HIPCHK(hipMemcpyAsync(Qt, e.Qt, (size_t)nx * nx * 8, hipMemcpyHostToDevice, h->stream));
  PF_HIPCHK(hipMemcpyAsync(Rt, e.Rt, (size_t)nz * nz * 8, hipMemcpyHostToDevice, h->stream));
  PF_HIPCHK(hipMemcpyAsync(xf, x0, nx * 8, hipMemcpyDeviceToDevice, h->stream));
  PF_HIPCHK(hipMemcpyAsync(Pf, P0, (size_t)nx * nx * 8, hipMemcpyDeviceToDevice, h->stream));
  PF_HIPCHK(hipEventCreateWithFlags(r.uploaded.out(), hipEventDisableTiming));
  PF_HIPCHK(hipEventRecord(r.uploaded, h->stream));
  PF_HIPCHK(hipStreamWaitEvent(h->side, r.uploaded, 0));
  r.cbeg = run_chunk_starts(r.T);
  r.ready.reserve(r.cbeg.size());
  for (size_t k = 0; k < r.cbeg.size(); ++k) {
    const int64_t c0 = r.cbeg[k], n = (k + 1 < r.cbeg.size() ? r.cbeg[k + 1] : r.T) - c0;
    PF_HIPCHK(h->ops->ekf(h->Pm, xf, Pf, Qt, Rt, r.dZ + c0 * nz, n, r.dP + c0 * nx * nx, xf, Pf,
                          r.edh ? r.dX + c0 * nx : nullptr, h->side));
    if (pf_status st = run_tables(r, c0, n, h->side); st != PF_OK) return st;
    pf::Event ev;
    PF_HIPCHK(hipEventCreateWithFlags(ev.out(), hipEventDisableTiming));
    PF_HIPCHK(hipEventRecord(ev, h->side));
    r.ready.push_back(std::move(ev));
  }
  return PF_OK;
}

// one step of the kernel chain (PF_LEDH_FUSED=0, grids that do not fit, nonlinear h)
pf_status run_step_chain(const Run& r, int64_t t) {
  pf_ledh_handle* h = r.h;
  if (pf_status st = enqueue_flow(h, r.dP + t * r.nx * r.nx, r.dZ + t * r.nz, r.u_at(t), r.noise, r.noise_at(t),
                                  nullptr, r.de + t, r.df + t, r.dTab ? r.dTab + t * r.tsz : nullptr);
      st != PF_OK)
    return st;
  return enqueue_finish(h, r.unif_at(t), r.mean_at(t), r.cov_at(t));
}

// The fused path: launch t flows step t and also reduces step t - 1's moments (its P5'), so a
// P5-only launch ends the run.  Between the launches the moment shifts are the MeanRing over mbuf,
// and the particle state is (the last step's flow rows, ancestors): xa holds the rows the next step
// starts from, xb takes its flow rows.
struct FusedSteps {
  const Run& r;
  pf_ledh_handle* h;
  double* const mbuf[3];  // what the ring's indices mean: {mean_prev, mean, mean3} at the start of the run
  MeanRing ring;
  double *xa, *xb;
  explicit FusedSteps(const Run& run)
      : r(run), h(run.h), mbuf{h->mean_prev, h->mean, h->mean3}, xa(h->x), xb(h->x_alt) {}

  // a launch's share of the handle: barrier words and phase, geometry, the moment-partial pair
  void handle_part(FusedParams& fp) {
    fp.stat = h->stat;
    fp.part = h->fpart;
    // moment partials: P5' reads the pair's buffer the previous step's P4 wrote, P4 the other
    const size_t cps = (size_t)FMAX * h->ops->fused_E;
    fp.cpart5 = h->fcpart + h->fcp * cps;
    fp.cpart = h->fcpart + (h->fcp ^ 1) * cps;
    if (fp.step) h->fcp ^= 1;
    fp.err = h->ferr;
    fp.phase0 = h->fphase;
    h->fphase += 4;
    fp.ratio = h->ratio;
    fp.nbk = h->fused_nbk;
    fp.ppb = h->fused_ppb;
  }
  // P5' of the launch after step t: step t's moments, shifted as step t was
  void moments_of(FusedParams& fp, int64_t t) {
    fp.p5 = 1;
    fp.shift5 = mbuf[ring.prev_shift];
    fp.mean5 = mbuf[ring.write];
    fp.o_mean5 = r.mean_at(t);
    fp.o_cov5 = r.cov_at(t);
  }
  pf_status step(int64_t t) {
    FusedParams fp{};
    fp.f = flow_params(h, r.dP + t * r.nx * r.nx, r.dZ + t * r.nz, r.u_at(t), r.noise, r.noise_at(t), nullptr);
    fp.f.table = r.dTab + t * r.tsz;
    fp.f.x_in = xa;
    fp.f.x_out = xb;
    fp.anc_in = t > 0 ? h->fanc : nullptr;
    fp.anc_out = h->fanc;
    fp.rp_unif = r.unif_at(t);
    fp.f.epoch = ++h->epoch;
    fp.ep_res = ++h->epoch;
    fp.w_out = h->w_alt;
    fp.step = 1;
    if (t > 0) moments_of(fp, t - 1);
    fp.shift = mbuf[ring.shift];
    fp.o_ess = r.de + t;
    fp.o_flag = r.df + t;
    handle_part(fp);
    PF_HIPCHK(h->ops->fused(fp, h->stream));
    std::swap(h->w, h->w_alt);
    std::swap(xa, xb);
    ring.advance(t);
    return PF_OK;
  }
  // the last step's outputs and the materialised state; commits the ring into the handle
  pf_status tail() {
    FusedParams fp{};
    fp.f.N = h->N;
    fp.f.Npad = h->Npad;
    fp.f.x_in = xa;
    fp.anc_in = h->fanc;
    fp.x_res = xb;
    if (xb != h->x) std::swap(h->x, h->x_alt);  // x = xb, x_alt = xa
    fp.step = 0;
    moments_of(fp, r.T - 1);
    handle_part(fp);
    PF_HIPCHK(h->ops->fused(fp, h->stream));
    int src[3];
    ring.commit(src);
    DevBuf<double> was[3] = {std::move(h->mean_prev), std::move(h->mean), std::move(h->mean3)};
    h->mean_prev = std::move(was[src[0]]);
    h->mean = std::move(was[src[1]]);
    h->mean3 = std::move(was[src[2]]);
    return PF_OK;
  }
};

// stage: the per-step body, the fused launches with their tail or the kernel chain
pf_status run_steps(const Run& r) {
  FusedSteps fused(r);
  const bool one_launch = r.fused();
  size_t next_chunk = 0;
  for (int64_t t = 0; t < r.T; ++t) {
    if (r.ekf && next_chunk < r.cbeg.size() && t == r.cbeg[next_chunk])
      PF_HIPCHK(hipStreamWaitEvent(r.h->stream, r.ready[next_chunk++], 0));
    if (pf_status st = one_launch ? fused.step(t) : run_step_chain(r, t); st != PF_OK) return st;
  }
  return one_launch ? fused.tail() : PF_OK;
}

// test hook (pf_hooks.h): PF_TEST_LEDH_FAIL=1 reports the fused grid barrier as timed out after a
// completed run
bool test_barrier_fail() { return pf::test_hook("PF_TEST_LEDH_FAIL"); }

// stage: the verdict of the finished run, the fused step's barrier word
pf_status run_verdict(const Run& r) {
  pf_ledh_handle* h = r.h;
  if (r.ekf) PF_HIPCHK(hipStreamSynchronize(h->side));
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  if (!h->ferr) return PF_OK;
  unsigned int fe = 0;
  PF_HIPCHK(hipMemcpy(&fe, h->ferr, 4, hipMemcpyDeviceToHost));
  if (fe == 0u && !test_barrier_fail()) return PF_OK;
  PF_HIPCHK(hipMemset(h->ferr, 0, 8));
  return fail(PF_E_HIP, "run: fused step grid barrier timed out (workgroups not co-resident)");
}

// stage: the outputs to the host, each optional
pf_status run_download(const Run& r, double* means, double* covs, double* ess, uint8_t* flags) {
  const int nx = r.nx;
  const int64_t T = r.T;
  std::vector<int32_t> fl((size_t)T);
  if (means) PF_HIPCHK(hipMemcpy(means, r.dm, (size_t)T * nx * 8, hipMemcpyDeviceToHost));
  if (covs) PF_HIPCHK(hipMemcpy(covs, r.dc, (size_t)T * nx * nx * 8, hipMemcpyDeviceToHost));
  if (ess) PF_HIPCHK(hipMemcpy(ess, r.de, (size_t)T * 8, hipMemcpyDeviceToHost));
  PF_HIPCHK(hipMemcpy(fl.data(), r.df, (size_t)T * 4, hipMemcpyDeviceToHost));
  if (r.ekf && r.ekf->x_final)
    PF_HIPCHK(hipMemcpy(r.ekf->x_final, r.dE + r.slot.x_final, nx * 8, hipMemcpyDeviceToHost));
  if (r.ekf && r.ekf->P_final)
    PF_HIPCHK(hipMemcpy(r.ekf->P_final, r.dE + r.slot.P_final, (size_t)nx * nx * 8, hipMemcpyDeviceToHost));
  if (flags)
    for (int64_t t = 0; t < T; ++t) flags[t] = fl[t] ? 1 : 0;
  return PF_OK;
}

pf_status run_impl(pf_ledh_handle* h, const double* Ps, const double* Xb, const EkfSpec* ekf, const double* Z,
                   const double* U, int64_t T, int32_t noise, double* means, double* covs, double* ess,
                   uint8_t* flags) {
  if (pf_status st = run_ready(h, Ps, Xb, ekf, Z, T, noise); st != PF_OK) return st;
  if (T <= 0) return PF_OK;
  PF_HIPCHK(hipSetDevice(h->device));
  Run r(h, Ps, Xb, ekf, Z, U, T, noise);
  if (pf_status st = run_carve(r); st != PF_OK) return st;
  // Up to here a return leaves the handle as it was.  From the first upload on, every exit ends the
  // pending resample decision and consumes the replay source (it serves one run), failed or not.
  bool stepped = false;
  pf_status st = run_upload(r);
  if (st == PF_OK) st = ekf ? run_tracker_ahead(r) : run_tables_upfront(r);
  if (st == PF_OK) {
    std::optional<GridOrderScope> order;  // no overlap with another handle's grid
    if (r.fused()) order.emplace(h->device, h->stream);
    stepped = true;
    st = run_steps(r);
    if (order) order->end();
  }
  if (st == PF_OK) st = run_verdict(r);
  if (st == PF_OK) st = run_download(r, means, covs, ess, flags);
  h->pending = false;
  h->rp_T = 0;
  // Once a step was enqueued, a failed launch or a timed-out grid barrier leaves x / anc / w / the
  // moment shifts part-advanced: the handle then reports 'not initialized' instead of continuing
  // from a corrupt state.
  if (st != PF_OK && stepped) h->initialized = false;
  return st;
}

}  // namespace

extern "C" {

pf_status pf_ledh_run(pf_ledh_handle* h, const double* Ps, const double* Z, const double* U, int64_t T, int32_t noise,
                      double* means, double* covs, double* ess, uint8_t* flags) try {
  if (!Ps) return fail(PF_E_ARG, "null argument");
  if (h && h->algo == 1) return fail(PF_E_ARG, "EDH handle: use pf_edh_run (it needs the tracker's past means)");
  return run_impl(h, Ps, nullptr, nullptr, Z, U, T, noise, means, covs, ess, flags);
} catch (...) { return pf::on_exception("pf_ledh_run"); }

pf_status pf_edh_run(pf_ledh_handle* h, const double* Ps, const double* Xbars, const double* Z, const double* U,
                     int64_t T, int32_t noise, double* means, double* covs, double* ess, uint8_t* flags) try {
  if (!Ps || !Xbars) return fail(PF_E_ARG, "null argument");
  if (h && h->algo != 1) return fail(PF_E_ARG, "pf_edh_run needs a handle from pf_edh_create");
  return run_impl(h, Ps, Xbars, nullptr, Z, U, T, noise, means, covs, ess, flags);
} catch (...) { return pf::on_exception("pf_edh_run"); }

pf_status pf_ledh_run_ekf(pf_ledh_handle* h, const double* x0, const double* P0, const double* Qt, const double* Rt,
                          const double* Z, const double* U, int64_t T, int32_t noise, double* means, double* covs,
                          double* ess, uint8_t* flags, double* x_final, double* P_final) try {
  if (!x0 || !P0 || !Qt || !Rt) return fail(PF_E_ARG, "null argument");
  EkfSpec e{x0, P0, Qt, Rt, x_final, P_final};
  return run_impl(h, nullptr, nullptr, &e, Z, U, T, noise, means, covs, ess, flags);
} catch (...) { return pf::on_exception("pf_ledh_run_ekf"); }

pf_status pf_ledh_ekf_sequence(pf_ledh_handle* h, const double* x0, const double* P0, const double* Qt,
                               const double* Rt, const double* Z, int64_t T, double* Ps, double* x_final,
                               double* P_final) try {
  if (!h || !x0 || !P0 || !Qt || !Rt || !Z) return fail(PF_E_ARG, "null argument");
  if (T <= 0) return PF_OK;
  PF_HIPCHK(hipSetDevice(h->device));
  const int nx = h->nx, nz = h->nz;
  const EkfSlots slot(nx, nz);
  DevBuf<double> dE, dZ, dP;  // freed on every return
  PF_HIPCHK(dE.alloc(slot.ne));
  PF_HIPCHK(dZ.alloc((size_t)T * nz));
  PF_HIPCHK(dP.alloc((size_t)T * nx * nx));
  double *ex0 = dE + slot.x0, *eP0 = dE + slot.P0, *eQ = dE + slot.Qt, *eR = dE + slot.Rt;
  double *exf = dE + slot.x_final, *ePf = dE + slot.P_final;
  PF_HIPCHK(hipMemcpy(ex0, x0, nx * 8, hipMemcpyHostToDevice));
  PF_HIPCHK(hipMemcpy(eP0, P0, (size_t)nx * nx * 8, hipMemcpyHostToDevice));
  PF_HIPCHK(hipMemcpy(eQ, Qt, (size_t)nx * nx * 8, hipMemcpyHostToDevice));
  PF_HIPCHK(hipMemcpy(eR, Rt, (size_t)nz * nz * 8, hipMemcpyHostToDevice));
  PF_HIPCHK(hipMemcpy(dZ, Z, (size_t)T * nz * 8, hipMemcpyHostToDevice));
  PF_HIPCHK(h->ops->ekf(h->Pm, ex0, eP0, eQ, eR, dZ, T, dP, exf, ePf, nullptr, h->stream));
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  if (Ps) PF_HIPCHK(hipMemcpy(Ps, dP, (size_t)T * nx * nx * 8, hipMemcpyDeviceToHost));
  if (x_final) PF_HIPCHK(hipMemcpy(x_final, exf, nx * 8, hipMemcpyDeviceToHost));
  if (P_final) PF_HIPCHK(hipMemcpy(P_final, ePf, (size_t)nx * nx * 8, hipMemcpyDeviceToHost));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_ledh_ekf_sequence"); }

pf_status pf_ledh_set_run_replay(pf_ledh_handle* h, const double* noise, const double* uniforms, int64_t T) try {
  if (!h || !noise || !uniforms || T <= 0) return fail(PF_E_ARG, "null argument");
  PF_HIPCHK(hipSetDevice(h->device));
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  h->rp_T = 0;
  PF_HIPCHK(h->rp_noise.alloc((size_t)T * h->N * h->nx));
  PF_HIPCHK(h->rp_unif.alloc((size_t)T));
  PF_HIPCHK(hipMemcpy(h->rp_noise, noise, (size_t)T * h->N * h->nx * 8, hipMemcpyHostToDevice));
  PF_HIPCHK(hipMemcpy(h->rp_unif, uniforms, (size_t)T * 8, hipMemcpyHostToDevice));
  h->rp_T = T;
  return PF_OK;
} catch (...) { return pf::on_exception("pf_ledh_set_run_replay"); }

void* pf_ledh_stream(pf_ledh_handle* h) { return h ? (void*)h->stream : nullptr; }
pf_status pf_ledh_synchronize(pf_ledh_handle* h) try {
  if (!h) return fail(PF_E_ARG, "null argument");
  PF_HIPCHK(hipStreamSynchronize(h->stream));
  return PF_OK;
} catch (...) { return pf::on_exception("pf_ledh_synchronize"); }
int32_t pf_ledh_shared_path(pf_ledh_handle* h) { return (h && h->shared) ? 1 : 0; }

}  // extern "C"

#ifdef PF_STAMPS
// diagnostic build only: per-workgroup phase stamps of the last fused LEDH step
extern "C" int pf_debug_stamps_ledh(unsigned long long* out, int n) {
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(pf::ledh::g_ledh_stamps), (size_t)n * sizeof(unsigned long long));
}
// k_flow_wave_lr phase accumulators (workgroup 0): read (n <= 16) and clear
extern "C" int pf_debug_lr_acc(unsigned long long* out, int n, int clear) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(pf::ledh::g_lr_acc), (size_t)n * sizeof(unsigned long long)) != hipSuccess)
    return 1;
  if (clear) {
    static const unsigned long long zeros[16] = {};
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(pf::ledh::g_lr_acc), zeros, sizeof(zeros));
  }
  return 0;
}
#endif
