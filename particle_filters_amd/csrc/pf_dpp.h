// Wave-level exchanges and reductions on the DPP network (GFX9 DPP: quad_perm, row shifts,
// row mirrors, row_bcast) instead of LDS-crossbar shuffles (ds_bpermute): shared by the SIR step
// kernels (pf_kernels.h) and the LEDH / EDH flow kernels (pf_ledh_kernels.h).
#pragma once
#include <hip/hip_runtime.h>

namespace pf {

// ---------------------------------------------------------------------------
// Wave reductions on the DPP network (GFX9 DPP: quad_perm, row mirrors,
// row_bcast) instead of LDS-crossbar shuffles.  Fixed combination tree ->
// deterministic, identical in every workgroup.
// ---------------------------------------------------------------------------
template <int CTRL, int RM = 0xf>
__device__ __forceinline__ int dpp_i(int old, int v) {
  return __builtin_amdgcn_update_dpp(old, v, CTRL, RM, 0xf, false);
}
template <int CTRL, int RM = 0xf>
__device__ __forceinline__ float dpp_f(float old, float v) {
  return __int_as_float(dpp_i<CTRL, RM>(__float_as_int(old), __float_as_int(v)));
}
template <int CTRL, int RM = 0xf>
__device__ __forceinline__ double dpp_d(double old, double v) {
  const long long o = __double_as_longlong(old), x = __double_as_longlong(v);
  const int lo = dpp_i<CTRL, RM>((int)o, (int)x);
  const int hi = dpp_i<CTRL, RM>((int)(o >> 32), (int)(x >> 32));
  return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
// the same move where every lane's source is valid (quad_perm, row mirrors, row_newbcast; or rows
// outside RM whose result is not read): no initialising move of the destination's old value
template <int CTRL, int RM = 0xf>
__device__ __forceinline__ double dpp_mov_d(double v) {
  const long long x = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_mov_dpp((int)x, CTRL, RM, 0xf, true);
  const int hi = __builtin_amdgcn_mov_dpp((int)(x >> 32), CTRL, RM, 0xf, true);
  return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
enum : int {
  DPP_QP_1032 = 0xB1,
  DPP_QP_2301 = 0x4E,
  DPP_ROW_MIRROR = 0x140,
  DPP_ROW_HMIRROR = 0x141,
  DPP_ROW_BCAST15 = 0x142,
  DPP_ROW_BCAST31 = 0x143
};

// The fp32 stages are one DPP-modified ALU instruction each, on a tied register: lane i gets
// op(v[src(i)], v[i]), and a lane outside the row mask keeps its value.  The compiler pads no
// hazard inside an asm statement, so the wait states stand in the strings: two between a VALU write
// of a register and a DPP read of it (s_nop 1; where independent stages are interleaved the other
// values' instructions take their place), and again before v_readlane reads the last stage.  The
// first s_nop covers a write of the operand by the instruction just ahead of the statement (a
// transcendental's result needs one wait state before any other VALU instruction reads it).
// All 64 lanes must be active: a lane whose DPP source is inactive keeps its value here, where the
// builtin form with an initialised `old` combined it with the identity (-0 + 0 = +0).
#define PF_DPP_QP1032 " quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
#define PF_DPP_QP2301 " quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
#define PF_DPP_HMIRROR " row_half_mirror row_mask:0xf bank_mask:0xf\n\t"
#define PF_DPP_MIRROR " row_mirror row_mask:0xf bank_mask:0xf\n\t"
#define PF_DPP_BCAST15 " row_bcast:15 row_mask:0xa bank_mask:0xf\n\t"
#define PF_DPP_BCAST31 " row_bcast:31 row_mask:0xc bank_mask:0xf\n\t"
// one value's four stages inside a row / its two stages across rows, each behind its wait states
#define PF_DPP_ROW1(OP, R)                                                                      \
  "s_nop 1\n\t" OP " " R ", " R ", " R PF_DPP_QP1032 "s_nop 1\n\t" OP " " R ", " R ", " R PF_DPP_QP2301 \
  "s_nop 1\n\t" OP " " R ", " R ", " R PF_DPP_HMIRROR "s_nop 1\n\t" OP " " R ", " R ", " R PF_DPP_MIRROR
#define PF_DPP_WAVE1(OP, R) \
  "s_nop 1\n\t" OP " " R ", " R ", " R PF_DPP_BCAST15 "s_nop 1\n\t" OP " " R ", " R ", " R PF_DPP_BCAST31
// one stage of three independent values: each value's next stage is two instructions behind its last
#define PF_DPP_STAGE3(OP, CTRL) OP " %0, %0, %0" CTRL OP " %1, %1, %1" CTRL OP " %2, %2, %2" CTRL

// every lane of each 16-lane row gets its row's result (the closing s_nop: the caller's next
// instruction may be a DPP read of it).  The fp64 forms stay builtins with an initialised `old`:
// where the argument is a product the compiler contracts their first add into an fma, which is part
// of the filters' bits, and another formulation (dpp_mov_d) moves which call sites it contracts.
// row_max_f, row_sum_f and wave_sum_u have no caller in a filter kernel at present (wave_max_u holds
// its own six stages, the resident step sums through wave_sum_prod_u3): they are the plain forms of
// the tree, kept for the kernels to come and run by the test entry pf_test_wave_reduce.
__device__ __forceinline__ float row_max_f(float v) {
  asm volatile(PF_DPP_ROW1("v_max_f32_dpp", "%0") "s_nop 1" : "+v"(v));
  return v;
}
__device__ __forceinline__ float row_sum_f(float v) {
  asm volatile(PF_DPP_ROW1("v_add_f32_dpp", "%0") "s_nop 1" : "+v"(v));
  return v;
}
__device__ __forceinline__ double row_sum_d(double v) {
  v += dpp_d<DPP_QP_1032>(0.0, v);
  v += dpp_d<DPP_QP_2301>(0.0, v);
  v += dpp_d<DPP_ROW_HMIRROR>(0.0, v);
  v += dpp_d<DPP_ROW_MIRROR>(0.0, v);
  return v;
}
__device__ __forceinline__ float lane63_f(float v) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ double lane63_d(double v) {
  const long long x = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)x, 63), hi = __builtin_amdgcn_readlane((int)(x >> 32), 63);
  return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
// lane L's value (L uniform) in every lane
__device__ __forceinline__ double readlane_d(double v, int L) {
  const long long x = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readlane((int)x, L), hi = __builtin_amdgcn_readlane((int)(x >> 32), L);
  return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo));
}
// whole-wave results (uniform: scalar registers).  Only lane 63 is read: after the row broadcasts
// rows 0 and 2 do not hold the wave's result.
__device__ __forceinline__ float wave_max_u(float v) {
  float r;
  asm volatile(PF_DPP_ROW1("v_max_f32_dpp", "%1") PF_DPP_WAVE1("v_max_f32_dpp", "%1")
               "s_nop 1\n\tv_readlane_b32 %0, %1, 63"
               : "=s"(r), "+v"(v));
  return r;
}
__device__ __forceinline__ float wave_sum_u(float v) {
  float r;
  asm volatile(PF_DPP_ROW1("v_add_f32_dpp", "%1") PF_DPP_WAVE1("v_add_f32_dpp", "%1")
               "s_nop 1\n\tv_readlane_b32 %0, %1, 63"
               : "=s"(r), "+v"(v));
  return r;
}
// The sums of three independent products a * b, stage by stage: the other two values' instructions
// stand where each value's wait states would.  The first stage is fma(a, b, p[partner]) with
// p = round(a * b), not p + p[partner]: that is what `v = a * b; v += dpp(v)` has always
// contracted to in the resident step, and so part of its outputs' bits.  The other stages are adds.
__device__ __forceinline__ void wave_sum_prod_u3(float a0, float b0, float a1, float b1, float a2, float b2,
                                                 float& r0, float& r1, float& r2) {
  float t0, t1, t2;
  // the opening s_nop: a factor may come straight out of a transcendental (one wait state)
  asm volatile("s_nop 0\n\tv_mul_f32 %0, %6, %7\n\tv_mul_f32 %1, %8, %9\n\tv_mul_f32 %2, %10, %11\n\t"
               "v_mov_b32_dpp %0, %0" PF_DPP_QP1032 "v_mov_b32_dpp %1, %1" PF_DPP_QP1032
               "v_mov_b32_dpp %2, %2" PF_DPP_QP1032
               "v_fmac_f32 %0, %6, %7\n\tv_fmac_f32 %1, %8, %9\n\tv_fmac_f32 %2, %10, %11\n\t"
               PF_DPP_STAGE3("v_add_f32_dpp", PF_DPP_QP2301) PF_DPP_STAGE3("v_add_f32_dpp", PF_DPP_HMIRROR)
               PF_DPP_STAGE3("v_add_f32_dpp", PF_DPP_MIRROR) PF_DPP_STAGE3("v_add_f32_dpp", PF_DPP_BCAST15)
               PF_DPP_STAGE3("v_add_f32_dpp", PF_DPP_BCAST31)
               "v_readlane_b32 %3, %0, 63\n\tv_readlane_b32 %4, %1, 63\n\tv_readlane_b32 %5, %2, 63"
               : "=&v"(t0), "=&v"(t1), "=&v"(t2), "=s"(r0), "=s"(r1), "=s"(r2)
               : "v"(a0), "v"(b0), "v"(a1), "v"(b1), "v"(a2), "v"(b2));
}
__device__ __forceinline__ double wave_sum_ud(double v) {
  v = row_sum_d(v);
  v += dpp_d<DPP_ROW_BCAST15, 0xa>(0.0, v);
  v += dpp_d<DPP_ROW_BCAST31, 0xc>(0.0, v);
  return lane63_d(v);
}
__device__ __forceinline__ double wave_max_ud(double v) {
  v = fmax(v, dpp_d<DPP_QP_1032>(-INFINITY, v));
  v = fmax(v, dpp_d<DPP_QP_2301>(-INFINITY, v));
  v = fmax(v, dpp_d<DPP_ROW_HMIRROR>(-INFINITY, v));
  v = fmax(v, dpp_d<DPP_ROW_MIRROR>(-INFINITY, v));
  v = fmax(v, dpp_d<DPP_ROW_BCAST15, 0xa>(-INFINITY, v));
  v = fmax(v, dpp_d<DPP_ROW_BCAST31, 0xc>(-INFINITY, v));
  return lane63_d(v);
}

// Inclusive wave scan on the DPP network (row_shr 1/2/4/8 within 16-lane rows, then the row
// broadcasts): no LDS crossbar round trips.  A fixed order, identical in every workgroup.
__device__ __forceinline__ double wave_incl_scan_dpp(double v) {
  v += dpp_d<0x111>(0.0, v);  // row_shr:1
  v += dpp_d<0x112>(0.0, v);  // row_shr:2
  v += dpp_d<0x114>(0.0, v);  // row_shr:4
  v += dpp_d<0x118>(0.0, v);  // row_shr:8
  v += dpp_d<DPP_ROW_BCAST15, 0xa>(0.0, v);
  v += dpp_d<DPP_ROW_BCAST31, 0xc>(0.0, v);
  return v;
}

// Exchanges inside aligned 4-lane groups (quad_perm): the lane-group flow's neighbours and sums
enum : int {
  DPP_QP_ROT1 = 0x39,  // lane q reads lane (q + 1) & 3: quad_perm [1, 2, 3, 0]
  DPP_QP_ROT3 = 0x93   // lane q reads lane (q + 3) & 3: quad_perm [3, 0, 1, 2]
};
__device__ __forceinline__ double quad_sum_d(double v) {
  v += dpp_d<DPP_QP_1032>(0.0, v);
  return v + dpp_d<DPP_QP_2301>(0.0, v);
}

}  // namespace pf
