// The shape and LDS layout of the one-launch Sinkhorn solver (pf_ot_resident.h: k_ot_resident), stated
// once for the kernel, for the host that sizes its dynamic LDS and answers pf_ot_resident_supported,
// and for the stand-alone check tests/host/pf_ot_resident_plan_check.cpp.
//
// One workgroup of RES_THREADS lanes (RES_WAVES waves, four per SIMD) solves one problem of N <=
// RES_MAXN particles with its cost matrix C [N][npad] in LDS.  The f pass gives every wave whole rows
// of C (lanes along the row).  The g pass keeps lanes along j as well, so that both passes read C
// along its rows, 8 bytes per lane at consecutive addresses: conflict-free.  Its npad / 64 column
// waves leave S = RES_WAVES / (npad / 64) waves per column, which split the source range into S
// chunks of `chunk` rows; the (max, sum, argmax) partials [S][npad] go through LDS and are merged in the
// order s = 0 .. S - 1.  The block reductions (the weight sum, the plan statistics) use RES_THREADS
// doubles that alias the partials, which are dead at those times.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pf_dpf_plan.h"

namespace pf {
namespace ot {

constexpr int RES_MAXN = 128;
constexpr int RES_THREADS = 1024;
constexpr int RES_WAVES = RES_THREADS / 64;
constexpr uint32_t RES_LDS_MAX = 163840;  // the LDS of one CU

struct ResidentPlan {
  int N, npad;
  int ncw;    // column waves of the g pass: npad / 64
  int S;      // splits of its source range
  int chunk;  // rows per split: ceil(N / S)
  // byte offsets into the dynamic LDS, each a multiple of 8
  uint32_t C;                          // [N][npad] doubles
  uint32_t a, f, g, fold, gold, x2;    // [npad] doubles each
  uint32_t pm, ps;                     // [S][npad] doubles each
  uint32_t pam;                        // [S][npad] int32
  uint32_t flag;                       // 2 int32: the stopping verdict
  uint32_t red;                        // [RES_THREADS] doubles, inside pm .. ps
  uint32_t total;
  bool fits;  // 1 <= N <= RES_MAXN and total <= RES_LDS_MAX
};

__host__ __device__ inline ResidentPlan resident_plan(int N) {
  ResidentPlan p{};
  p.N = N;
  p.fits = N >= 1 && N <= RES_MAXN;
  if (!p.fits) return p;
  p.npad = (N + dpf::CB - 1) / dpf::CB * dpf::CB;  // dpf::npad, which is host-only
  p.ncw = p.npad / 64;
  p.S = RES_WAVES / p.ncw;
  p.chunk = (N + p.S - 1) / p.S;
  const uint32_t vec = (uint32_t)p.npad * 8, part = (uint32_t)p.S * (uint32_t)p.npad;
  uint32_t o = 0;
  p.C = o, o += (uint32_t)N * vec;
  p.a = o, o += vec;
  p.f = o, o += vec;
  p.g = o, o += vec;
  p.fold = o, o += vec;
  p.gold = o, o += vec;
  p.x2 = o, o += vec;
  p.pm = o, o += part * 8;
  p.ps = o, o += part * 8;
  p.pam = o, o += part * 4;
  p.flag = o, o += 8;
  p.red = p.pm;
  p.total = o;
  p.fits = p.total <= RES_LDS_MAX && 2 * part * 8 >= (uint32_t)RES_THREADS * 8;
  return p;
}

}  // namespace ot
}  // namespace pf
