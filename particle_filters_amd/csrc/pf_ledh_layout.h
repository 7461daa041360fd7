// LEDH / EDH layouts with nx / nz as values, shared by the kernels (pf_ledh_kernels.h expresses
// Lay<NX, NZ> and TLay<NX, NZ>::size through this) and the host (pf_ledh.hip fills the parameter
// block and sizes the flow table from it).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace pf {
namespace ledh {

struct LedhLay {
  // parameter block (doubles), Lay<NX, NZ>
  int A;     // nx*nx transition matrix (LINEAR g)
  int EX;    // F, dt (L96 g)
  int H;     // nz*nx observation matrix (LINEAR h)
  int C;     // nz offset (LINEAR) / beta (EXP_HALF)
  int AC;    // psi, d0, sx[nz], sy[nz] (ACOUSTIC)
  int LQ;    // nx*nx chol(Q) (device noise)
  int QI;    // nx*nx Q^{-1}
  int R;     // nz*nz R
  int RI;    // nz*nz R^{-1}
  int SIZE;
  // shared-path flow table (doubles), TLay<NX, NZ>: head, one block per lambda step, composed flow
  int THEAD, TPJ, TAFF;
  int EDH;   // the EDH general map that may take the composed flow's place (ELay<NX>::SIZE)
  __host__ __device__ constexpr LedhLay(int nx, int nz)
      : A(0),
        EX(A + nx * nx),
        H(EX + 2),
        C(H + nz * nx),
        AC(C + nz),
        LQ(AC + 2 + 2 * nz),
        QI(LQ + nx * nx),
        R(QI + nx * nx),
        RI(R + nz * nz),
        SIZE(RI + nz * nz),
        THEAD(nx + nz),
        TPJ(nx * nz + nz * nz + nx + nz + 1),
        TAFF(nx + nx * nz + nz + nz * nz + 1),
        EDH(nx * nx + nx) {}
  __host__ __device__ constexpr int aff(int L) const { return THEAD + L * TPJ; }
  __host__ __device__ constexpr int size(int L) const { return aff(L) + TAFF; }  // TLay<NX, NZ>::size(L)
  // doubles of the table the host allocates: its last block holds the composed flow or the EDH map
  constexpr size_t table_size(int L) const {
    return (size_t)THEAD + (size_t)L * (size_t)TPJ + (size_t)(TAFF > EDH ? TAFF : EDH);
  }
};

}  // namespace ledh
}  // namespace pf
