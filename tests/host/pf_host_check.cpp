// Stand-alone check of the host support header (particle_filters_amd/csrc/pf_host.h) and of the
// LEDH layout (pf_ledh_layout.h), test infrastructure only.  Built with the host sanitizers by
// `make -C particle_filters_amd/csrc hostcheck`; runs without a GPU (it hides every device, so
// DevBuf::alloc fails the same way everywhere).  Prints "ok" and exits 0, or names what failed.
#include <cstdio>
#include <cstdlib>
#include <new>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../particle_filters_amd/csrc/pf_edh_kernels.h"
#include "../../particle_filters_amd/csrc/pf_host.h"
#include "../../particle_filters_amd/csrc/pf_ledh_kernels.h"

static std::string g_msg;
namespace pf {
void set_last_error(const std::string& msg) { g_msg = msg; }
}  // namespace pf

// every shape of lregistry() (pf_ledh.hip): the host's runtime layout is the kernels' compiled one
template <int NX, int NZ>
constexpr bool lay_matches() {
  using namespace pf::ledh;
  constexpr LedhLay l(NX, NZ);
  using K = Lay<NX, NZ>;
  return l.A == K::A && l.EX == K::EX && l.H == K::H && l.C == K::C && l.AC == K::AC && l.LQ == K::LQ &&
         l.QI == K::QI && l.R == K::R && l.RI == K::RI && l.SIZE == K::SIZE && l.size(8) == TLay<NX, NZ>::size(8) &&
         l.aff(8) == TLay<NX, NZ>::aff(8) && l.table_size(8) >= (size_t)l.size(8) &&
         l.table_size(8) >= (size_t)l.aff(8) + ELay<NX>::SIZE;
}
static_assert(lay_matches<1, 1>(), "LedhLay(1, 1)");
static_assert(lay_matches<2, 1>(), "LedhLay(2, 1)");
static_assert(lay_matches<4, 9>(), "LedhLay(4, 9)");
static_assert(lay_matches<4, 12>(), "LedhLay(4, 12)");
static_assert(lay_matches<4, 25>(), "LedhLay(4, 25)");
static_assert(lay_matches<16, 25>(), "LedhLay(16, 25)");
static_assert(lay_matches<40, 10>(), "LedhLay(40, 10)");
// the offsets themselves, once, written out by hand (nx = 2, nz = 1)
static_assert(pf::ledh::LedhLay(2, 1).EX == 4 && pf::ledh::LedhLay(2, 1).H == 6 && pf::ledh::LedhLay(2, 1).C == 8 &&
                  pf::ledh::LedhLay(2, 1).AC == 9 && pf::ledh::LedhLay(2, 1).LQ == 13 && pf::ledh::LedhLay(2, 1).QI == 17 &&
                  pf::ledh::LedhLay(2, 1).R == 21 && pf::ledh::LedhLay(2, 1).RI == 22 && pf::ledh::LedhLay(2, 1).SIZE == 23,
              "LedhLay(2, 1) offsets");
// (40, 10): the EDH map (nx * nx + nx = 1640) is the larger last block of the allocated table
static_assert(pf::ledh::LedhLay(40, 10).table_size(8) == 50 + 8 * 551 + 1640, "LedhLay(40, 10) table");

static int g_bad = 0;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_bad;                                                     \
    }                                                              \
  } while (0)

// entries shaped like the library's extern "C" functions
extern "C" pf_status entry_bad_alloc(int n) try {
  if (n) throw std::bad_alloc();
  return PF_OK;
} catch (...) {
  return pf::on_exception("entry_bad_alloc");
}
extern "C" pf_status entry_runtime_error(int n) try {
  std::vector<int> v((size_t)n);
  if (n) throw std::runtime_error("boom");
  return PF_OK;
} catch (...) {
  return pf::on_exception("entry_runtime_error");
}
static pf_status entry_hipchk() {
  PF_HIPCHK(hipErrorInvalidValue);
  return PF_OK;
}

static bool eq(const std::vector<double>& a, std::initializer_list<double> b) {
  return a == std::vector<double>(b);
}

int main() {
  setenv("HIP_VISIBLE_DEVICES", "-1", 1);  // no device, wherever this runs
  setenv("ROCR_VISIBLE_DEVICES", "-1", 1);

  // ---- exception boundary and error helpers
  g_msg.clear();
  CHECK(entry_bad_alloc(0) == PF_OK && g_msg.empty());
  CHECK(entry_bad_alloc(1) == PF_E_HIP);
  CHECK(g_msg.find("entry_bad_alloc") != std::string::npos);
  CHECK(entry_runtime_error(3) == PF_E_HIP);
  CHECK(g_msg.find("entry_runtime_error") != std::string::npos);
  CHECK(pf::fail(PF_E_ARG, "why") == PF_E_ARG && g_msg == "why");
  CHECK(entry_hipchk() == PF_E_HIP);
  CHECK(g_msg == std::string("hipErrorInvalidValue: ") + hipGetErrorString(hipErrorInvalidValue));

  // ---- linear algebra (every value dyadic: equality is exact)
  std::vector<double> L, Ai;
  const double A[4] = {4, 2, 2, 5};
  CHECK(pf::chol_lower(A, 2, 0.0, L) && eq(L, {2, 0, 1, 2}));
  CHECK(pf::spd_inverse(A, 2, Ai) && eq(Ai, {0.3125, -0.125, -0.125, 0.25}));
  const double B[4] = {1, 2, 2, 1};
  CHECK(!pf::chol_lower(B, 2, 0.0, L));
  CHECK(!pf::spd_inverse(B, 2, Ai));
  const double Z[1] = {0};
  CHECK(!pf::chol_lower(Z, 1, 0.0, L));
  CHECK(pf::chol_lower(Z, 1, 1e-10, L) && L.size() == 1 && L[0] == std::sqrt(1e-10));
  const double N1[1] = {-1};
  CHECK(!pf::chol_lower(N1, 1, 0.0, L));
  const double I1[1] = {4};
  CHECK(pf::chol_lower(I1, 1, 0.0, L) && eq(L, {2}));
  CHECK(pf::spd_inverse(I1, 1, Ai) && eq(Ai, {0.25}));
  const double J[4] = {0, 0, 0, 0};  // the jitter reaches the diagonal only
  CHECK(pf::chol_lower(J, 2, 4.0, L) && eq(L, {2, 0, 0, 2}));
  const double D[9] = {1, 0, 0, 0, 2, 0, 0, 0, 3}, ND[9] = {1, 0, 0, 0, 2, 0, 0, 1e-300, 3};
  CHECK(pf::is_diag(D, 3) && !pf::is_diag(ND, 3) && pf::is_diag(I1, 1) && !pf::is_diag(A, 2));

  // ---- DevBuf / Owned without a device
  {
    pf::DevBuf<double> b;
    CHECK(b.get() == nullptr && !b && (double*)b == nullptr);
    CHECK(b.alloc(16) != hipSuccess);
    CHECK(b.get() == nullptr);
    (void)hipGetLastError();
    b.reset();
    CHECK(b.get() == nullptr);
    pf::DevBuf<double> c(std::move(b));
    CHECK(c.get() == nullptr && b.get() == nullptr);
    b = std::move(c);
    std::swap(b, c);
    CHECK(c.get() == nullptr && b.get() == nullptr);
    pf::DevBuf<void> v;
    CHECK(v.alloc(64) != hipSuccess && v.get() == nullptr);
    (void)hipGetLastError();
    pf::Stream s;
    pf::Event e, e2(std::move(e));
    CHECK(!s && !e2 && !e);
    s.reset();
    CHECK((void*)s == nullptr);
    static_assert(!std::is_copy_constructible_v<pf::DevBuf<double>> && !std::is_copy_assignable_v<pf::DevBuf<double>> &&
                      !std::is_copy_constructible_v<pf::Stream>,
                  "the owners are move-only");
  }

  if (g_bad) return 1;
  std::printf("ok\n");
  return 0;
}
