// The two host rules that choose how an aggregation kernel addresses its tables (stag_amd/csrc/entry_args.hpp):
// narrow_rows (agg_half, agg_w1, agg_mc_edge, agg_mc_pedge) and agg_forms (agg_common of api.hip), at every boundary.
// Stand-alone: built and run by tests/test_address_forms_host.py, never loaded into another process.
//   address_forms                              the boundary table below; exit status 1 and a line per miss
//   address_forms rows n_src ldx D esize       -> "rc x_bytes"
//   address_forms agg n_src n_edges ldx D      -> "rc wide x_bytes idx_bytes"
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../stag_amd/csrc/entry_args.hpp"

namespace {

int misses = 0, checks = 0;

void expect(bool ok, const char* what, long long a, long long b, long long c, long long d) {
  ++checks;
  if (ok) return;
  ++misses;
  std::printf("MISS %s (%lld, %lld, %lld, %lld)\n", what, a, b, c, d);
}

constexpr int64_t k24 = 1ll << 24, k30 = 1ll << 30, k32 = 1ll << 32;

// narrow_rows(n_src, ldx, D, esize): rc and whether x_bytes names the narrow form (then it must be the extent)
void rows(int64_t n_src, int64_t ldx, int32_t D, uint32_t esize, int rc_want, bool narrow_want) {
  uint32_t xb = 0xDEADBEEFu;
  const int rc = stag::narrow_rows(n_src, ldx, D, esize, xb);
  const uint64_t extent = n_src > 0 ? ((uint64_t)(n_src - 1) * (uint64_t)ldx + (uint64_t)D) * esize : 0u;
  expect(rc == rc_want, "narrow_rows rc", n_src, ldx, D, esize);
  expect((xb != 0) == narrow_want, "narrow_rows form", n_src, ldx, D, esize);
  if (narrow_want) expect(xb == extent, "narrow_rows extent", n_src, ldx, D, esize);
}

// agg_forms(n_src, n_edges, ldx, D): rc, the two wide bits, and the extent behind the descriptor in the narrow form
void agg(int64_t n_src, int64_t n_edges, int64_t ldx, int32_t D, int rc_want, unsigned wide_want) {
  stag::AggForms f{7u, 7u, 7u};
  const int rc = stag::agg_forms(n_src, n_edges, ldx, D, f);
  expect(rc == rc_want, "agg_forms rc", n_src, n_edges, ldx, D);
  if (rc_want != STAG_OK) {
    expect(f.wide == 0 && f.x_bytes == 0 && f.idx_bytes == 0, "agg_forms refused: nothing set", n_src, n_edges, ldx, D);
    return;
  }
  expect(f.wide == wide_want, "agg_forms wide", n_src, n_edges, ldx, D);
  const uint64_t extent = ldx == 0 ? (uint64_t)D * 4u : (uint64_t)n_src * (uint64_t)ldx * 4u;
  expect(f.x_bytes == ((wide_want & 1u) ? 0u : (uint32_t)extent), "agg_forms x_bytes", n_src, n_edges, ldx, D);
  if (!(wide_want & 1u)) expect(extent < (1ull << 32), "agg_forms narrow extent fits", n_src, n_edges, ldx, D);
  expect(f.idx_bytes == (n_edges < k30 ? (uint32_t)n_edges * 4u : 0u), "agg_forms idx_bytes", n_src, n_edges, ldx, D);
}

int table() {
  // ---- rows: 2^24 - 1 | 2^24 --------------------------------------------------------------------------------
  rows(k24 - 1, 8, 8, 4, STAG_OK, true);
  rows(k24, 8, 8, 4, STAG_OK, false);
  rows(k24 - 1, 8, 8, 2, STAG_OK, true);
  rows(k24, 8, 8, 2, STAG_OK, false);
  agg(k24 - 1, 10, 8, 8, STAG_OK, 0);
  agg(k24, 10, 8, 8, STAG_OK, 1);
  // ---- stride: 2^24 - 4 | 2^24 bytes (halves: 2^24 - 2 | 2^24) ---------------------------------------------
  rows(6, (k24 - 4) / 4, 8, 4, STAG_OK, true);
  rows(6, k24 / 4, 8, 4, STAG_OK, false);
  rows(6, (k24 - 2) / 2, 8, 2, STAG_OK, true);
  rows(6, k24 / 2, 8, 2, STAG_OK, false);
  agg(6, 10, (k24 - 4) / 4, 8, STAG_OK, 0);
  agg(6, 10, k24 / 4, 8, STAG_OK, 1);
  // ---- extent: 2^32 - 4 | 2^32 bytes -------------------------------------------------------------------------
  // narrow_rows counts (n_src - 1) * ldx + D elements: 2^20 rows of 1024 floats end at 2^32 with D = 1024, 4 short of it with 1023
  rows(1ll << 20, 1024, 1023, 4, STAG_OK, true);
  rows(1ll << 20, 1024, 1024, 4, STAG_OK, false);
  rows(1ll << 20, 2048, 2047, 2, STAG_OK, true);     // 2^32 - 2 bytes of halves
  rows(1ll << 20, 2048, 2048, 2, STAG_OK, false);
  // agg_forms counts n_src * ldx floats: 2^30 - 1 of them (a prime-free way there: (2^15 - 1) rows of (2^15 + 1)) | 2^30
  agg((1ll << 15) - 1, 10, (1ll << 15) + 1, 8, STAG_OK, 0);
  agg(1ll << 15, 10, 1ll << 15, 8, STAG_OK, 1);
  agg(k24 - 1, 10, 64, 64, STAG_OK, 0);              // the top of the narrow form: 2^32 - 256 bytes
  agg(k24 - 1, 10, 65, 64, STAG_OK, 1);
  // ---- ldx == 0: one broadcast row (agg_forms: D floats behind the descriptor, whatever n_src) -----------------
  agg(5, 10, 0, 8, STAG_OK, 0);
  agg(k24 - 1, 10, 0, 8, STAG_OK, 0);
  agg(k24, 10, 0, 8, STAG_OK, 1);
  rows(5, 0, 8, 4, STAG_OK, true);                   // (its callers refuse ldx == 0 before the rule; the rule: D elements)
  rows(1, 0, 8, 2, STAG_OK, true);
  // ---- n_src == 0: nothing to address.  narrow_rows: no extent, so the 64-bit form; agg_forms: an empty descriptor ----
  rows(0, 8, 8, 4, STAG_OK, false);
  agg(0, 0, 8, 8, STAG_OK, 0);
  // ---- a stride of 2^32 bytes: refused by both, one element below it taken (wide) --------------------------------
  rows(3, k30, 8, 4, STAG_ENOSYS, false);
  rows(3, k30 - 1, 8, 4, STAG_OK, false);
  rows(3, k32 / 2, 8, 2, STAG_ENOSYS, false);
  rows(3, k32 / 2 - 1, 8, 2, STAG_OK, false);
  rows(1, k30, 8, 4, STAG_ENOSYS, false);
  agg(3, 10, k30, 8, STAG_ENOSYS, 0);
  agg(3, 10, k30 - 1, 8, STAG_OK, 1);
  agg(1, 10, k30, 8, STAG_ENOSYS, 0);
  agg(3, 10, 1ll << 40, 8, STAG_ENOSYS, 0);
  agg(3, 10, 1ll << 62, 8, STAG_ENOSYS, 0);          // (ldx * 4 would wrap in 64 bits)
  // ---- per-edge rows of agg_forms: 2^24 - 1 | 2^24 edges, n_edges * D * 4 = 2^32 - 4 * D | 2^32 ------------------
  agg(5, k24 - 1, 8, 8, STAG_OK, 0);
  agg(5, k24, 8, 8, STAG_OK, 2);
  agg(5, (1ll << 22) - 1, 256, 256, STAG_OK, 0);
  agg(5, 1ll << 22, 256, 256, STAG_OK, 2);
  agg(k24, k24, 8, 8, STAG_OK, 3);
  agg(5, k30 - 1, 8, 1, STAG_OK, 2);
  agg(5, k30, 8, 1, STAG_OK, 2);                     // idx_bytes: 0 from 2^30 edges on
  std::printf("%d checks, %d missed\n", checks, misses);
  return misses ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 1) return table();
  if (argc == 6 && !std::strcmp(argv[1], "rows")) {
    uint32_t xb = 0;
    const int rc = stag::narrow_rows(std::atoll(argv[2]), std::atoll(argv[3]), (int32_t)std::atoll(argv[4]),
                                     (uint32_t)std::atoll(argv[5]), xb);
    std::printf("%d %u\n", rc, xb);
    return 0;
  }
  if (argc == 6 && !std::strcmp(argv[1], "agg")) {
    stag::AggForms f{};
    const int rc = stag::agg_forms(std::atoll(argv[2]), std::atoll(argv[3]), std::atoll(argv[4]), (int32_t)std::atoll(argv[5]), f);
    std::printf("%d %u %u %u\n", rc, f.wide, f.x_bytes, f.idx_bytes);
    return 0;
  }
  std::fprintf(stderr, "usage: address_forms [rows n_src ldx D esize | agg n_src n_edges ldx D]\n");
  return 2;
}
