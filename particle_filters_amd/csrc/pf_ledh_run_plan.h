// Bookkeeping of one LEDH / EDH engine run (run_impl in pf_ledh.hip): where the run's buffers lie in
// the handle's arena, the slots of the device EKF block, the tracker-ahead chunk schedule and the
// rotation of the three moment-shift buffers of the fused step.  Host code only, no HIP, 64-bit
// sizes: tests/host/pf_ledh_run_plan_host_check.cpp runs it alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace pf {
namespace ledh {

// ---- EKF block (doubles): x0 | P0 | Qt | Rt | x_final | P_final
struct EkfSlots {
  size_t x0, P0, Qt, Rt, x_final, P_final;
  size_t ne;  // doubles of the whole block
  constexpr EkfSlots(int nx, int nz)
      : x0(0),
        P0(x0 + (size_t)nx),
        Qt(P0 + (size_t)nx * nx),
        Rt(Qt + (size_t)nx * nx),
        x_final(Rt + (size_t)nz * nz),
        P_final(x_final + (size_t)nx),
        ne(P_final + (size_t)nx * nx) {}
};

// ---- arena: the run's pieces in the order they lie, each on a 256-byte boundary
enum RunPiece {
  RUN_P,       // tracker covariances [T][nx][nx]
  RUN_Z,       // observations [T][nz]
  RUN_U,       // offsets [T][nx] (absent without U)
  RUN_MEANS,   // [T][nx]
  RUN_COVS,    // [T][nx][nx]
  RUN_ESS,     // [T]
  RUN_FLAGS,   // [T] int32
  RUN_EKF,     // EkfSlots block (device tracker)
  RUN_XBAR,    // EDH: tracker past means [T][nx]
  RUN_TABLES,  // flow tables [T][table doubles] (shared path and EDH)
  RUN_PIECES
};

struct RunArena {
  uint64_t bytes[RUN_PIECES];  // 0: the piece is absent
  uint64_t off[RUN_PIECES];
  uint64_t total;
  // the piece in the allocation at base, null when absent
  template <class T>
  T* at(char* base, RunPiece p) const {
    return bytes[p] ? reinterpret_cast<T*>(base + off[p]) : nullptr;
  }
};

inline RunArena run_arena(const uint64_t (&bytes)[RUN_PIECES]) {
  RunArena a{};
  for (int i = 0; i < RUN_PIECES; ++i) {
    a.bytes[i] = bytes[i];
    a.off[i] = a.total;
    a.total += (bytes[i] + 255) / 256 * 256;
  }
  return a;
}

// the piece sizes of a run of T steps; table_doubles is LedhLay(nx, nz).table_size(L)
inline RunArena run_arena(int nx, int nz, int64_t T, uint64_t table_doubles, bool has_U, bool ekf, bool edh,
                          bool tabled) {
  const uint64_t t = (uint64_t)T, x = (uint64_t)nx, z = (uint64_t)nz;
  uint64_t b[RUN_PIECES];
  b[RUN_P] = t * x * x * 8;
  b[RUN_Z] = t * z * 8;
  b[RUN_U] = has_U ? t * x * 8 : 0;
  b[RUN_MEANS] = t * x * 8;
  b[RUN_COVS] = t * x * x * 8;
  b[RUN_ESS] = t * 8;
  b[RUN_FLAGS] = t * 4;
  b[RUN_EKF] = ekf ? (uint64_t)EkfSlots(nx, nz).ne * 8 : 0;
  b[RUN_XBAR] = edh ? t * x * 8 : 0;
  b[RUN_TABLES] = tabled ? t * table_doubles * 8 : 0;
  return run_arena(b);
}

// ---- device tracker: the EKF and the flow tables run ahead of the particle loop in chunks of steps
// that grow 2, 4, 8, 16, 16, ... (the loop starts after two EKF steps, not sixteen).  The first step
// of each chunk over [0, T); chunk k ends where chunk k + 1 starts, the last one at T.
constexpr int64_t RUN_CHUNK_MAX = 16;
inline std::vector<int64_t> run_chunk_starts(int64_t T) {
  std::vector<int64_t> c;
  for (int64_t c0 = 0, n = 2; c0 < T; c0 += n, n = 2 * n < RUN_CHUNK_MAX ? 2 * n : RUN_CHUNK_MAX) c.push_back(c0);
  return c;
}

// ---- fused run: rotation of the three moment buffers, as indices into {mean_prev, mean, mean3} at
// the start of the run.  Launch t flows step t and reduces step t - 1's moments, so step t's shift is
// the mean of step t - 2, or the latest mean before the run (buffer 0) for t < 2: steps 0 and 1 both
// shift by it.  A launch never writes a buffer it reads: the write target is the third one.
struct MeanRing {
  int prev_shift = 0;  // the shift step t - 1 used (read with its partials)
  int shift = 0;       // the shift of step t
  int write = 1;       // where launch t puts the mean of step t - 1 (the tail: of step T - 1)
  // after launch t of the loop; the tail launch reads the ring as it then stands
  void advance(int64_t t) {
    if (t == 0) return;  // launch 0 reduced nothing: buffer `write` is still free
    const int freed = 3 - shift - write;
    prev_shift = shift;
    shift = write;
    write = freed;
  }
  // after the tail: src[i] is the run-start buffer that becomes mean_prev (i = 0), mean, mean3.  The
  // latest mean becomes mean_prev, the next moments' shift; the other two keep their order.
  void commit(int (&src)[3]) const {
    src[0] = write;
    src[1] = write == 0 ? 1 : 0;
    src[2] = write == 2 ? 1 : 2;
  }
};

}  // namespace ledh
}  // namespace pf
