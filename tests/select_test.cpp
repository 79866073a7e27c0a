// select_test.cpp -- the pure host functions that choose the tiled kernels (randomfield_amd/csrc/rf_select.h): which fast generation
// variant, which pass runs as Col2 halves, and which launches a fast generation pass makes.  Stand-alone: compiled with
// -fsanitize=address,undefined and run by tests/test_launch_select.py; exit status 0 = every check held.
#include <cstdio>
#include <vector>

#include "../randomfield_amd/csrc/rf_select.h"

namespace {
using namespace rf;

int g_failed = 0, g_checked = 0;
#define CHECK(cond)                                                              \
  do {                                                                           \
    ++g_checked;                                                                 \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++g_failed; } \
  } while (0)

// ---- fastgen_variant against the literal tables: the first rule whose conditions all hold decides -----------------------------------
// a condition: 1 = must be set, 0 = must be clear, -1 = either; `len`: 0 = any length, else that one
struct Rule { int emit, n64, n32, pot, slab, len; FastVariant out; };
const FastVariant INV{false, 0, 0, 0, false};
constexpr FastVariant W(int slab, int pot, int src) { return FastVariant{true, slab, pot, src, false}; }
constexpr FastVariant H(int pot) { return FastVariant{true, 0, pot, 0, true}; }
const Rule kRules32[] = {
    {1, -1, -1, -1, 1, 0, INV},      {1, -1, -1, 1, -1, 0, INV},     {1, 1, -1, -1, -1, 0, INV},   // emit: slab, pot or noise64
    {1, -1, 1, -1, -1, 0, W(0, 2, 2)}, {1, -1, -1, -1, -1, 2048, H(2)}, {1, -1, -1, -1, -1, 0, W(0, 2, 0)},
    {-1, 1, -1, -1, 1, 0, INV},      {-1, 1, -1, 1, -1, 0, INV},     {-1, 1, -1, -1, -1, 0, W(0, 0, 1)},     // noise64
    {-1, -1, 1, -1, 1, 0, INV},      {-1, -1, 1, 1, -1, 0, W(0, 1, 2)}, {-1, -1, 1, -1, -1, 0, W(0, 0, 2)},   // noise32
    {-1, -1, -1, 1, 1, 0, INV},      {-1, -1, -1, 1, -1, 0, W(0, 1, 0)},                                   // pot
    {-1, -1, -1, -1, 1, 0, W(1, 0, 0)},                                                                    // slab
    {-1, -1, -1, -1, -1, 2048, H(0)}, {-1, -1, -1, -1, -1, 0, W(0, 0, 0)},
};
const Rule kRules64[] = {
    {-1, -1, -1, -1, -1, 2048, INV},                                                                       // does not fit the LDS
    {-1, 1, -1, -1, -1, 0, INV},     {-1, -1, 1, -1, -1, 0, INV},                                          // any resident noise
    {1, -1, -1, -1, 1, 0, INV},      {1, -1, -1, 1, -1, 0, INV},     {1, -1, -1, -1, -1, 1024, H(2)}, {1, -1, -1, -1, -1, 0, W(0, 2, 0)},
    {-1, -1, -1, 1, 1, 0, INV},      {-1, -1, -1, 1, -1, 0, W(0, 1, 0)},                                   // pot, N = 1024 included
    {-1, -1, -1, -1, 0, 1024, H(0)},
    {-1, -1, -1, -1, 1, 0, W(1, 0, 0)}, {-1, -1, -1, -1, -1, 0, W(0, 0, 0)},
};
template <int NR> FastVariant by_table(const Rule (&rules)[NR], int N, int emit, int n64, int n32, int pot, int slab) {
  auto ok = [](int want, int have) { return want < 0 || want == have; };
  for (const Rule& r : rules)
    if (ok(r.emit, emit) && ok(r.n64, n64) && ok(r.n32, n32) && ok(r.pot, pot) && ok(r.slab, slab) && (r.len == 0 || r.len == N)) return r.out;
  return INV;
}
template <typename T> bool in_list(const FastVariant& v) {
  return with_fast_variant(FastListOf<T>{}, v, false, [](auto) { return true; });
}
void test_variants() {
  const int sizes[] = {8, 16, 32, 64, 128, 256, 512, 1024, 2048};
  int cases = 0;
  for (int f64 = 0; f64 < 2; ++f64)
    for (int N : sizes)
      for (int m = 0; m < 32; ++m) {
        const int emit = m & 1, n64 = (m >> 1) & 1, n32 = (m >> 2) & 1, pot = (m >> 3) & 1, slab = (m >> 4) & 1;
        const FastVariant got = fastgen_variant(f64, N, emit, n64, n32, pot, slab);
        const FastVariant want = f64 ? by_table(kRules64, N, emit, n64, n32, pot, slab) : by_table(kRules32, N, emit, n64, n32, pot, slab);
        if (!(got == want)) std::printf("  f64=%d N=%d emit=%d n64=%d n32=%d pot=%d slab=%d\n", f64, N, emit, n64, n32, pot, slab);
        CHECK(got == want);
        // what is chosen exists as a kernel (the launch path finds its entry), and only at a length that has it
        if (got.valid) CHECK(f64 ? in_list<double>(got) : in_list<float>(got));
        if (got.valid && got.halves) CHECK(N == fastgen_halves_length(f64));
        ++cases;
      }
  CHECK(cases == 576);
  for (int f64 = 0; f64 < 2; ++f64)
    for (int N : {0, 4, 100, 4096}) CHECK(!fastgen_variant(f64, N, false, false, false, false, false).valid);   // lengths that are not served
  CHECK(!in_list<double>(W(0, 0, 2)) && !in_list<float>(INV) && !in_list<float>(H(1)));
}

// ---- col_halves / halves_fit ---------------------------------------------------------------------------------------------------------
template <class C1> void test_fit() {
  ColGeom g{64, 64 * 8, 64};
  CHECK(halves_fit<C1>(g));
  // the half's rows are two rows of the column apart: 32-bit byte offsets up to ((LMAX - 1) * 2 * row_stride + TC) * 8 < 2^32
  const long long last = (((1LL << 32) - 1) / 8 - C1::TC) / (2 * (C1::LMAX - 1));
  g.row_stride = last;
  CHECK(halves_fit<C1>(g));
  g.row_stride = last + 1;
  CHECK(!halves_fit<C1>(g));
  g.row_stride = 64;
  ColGeom b = g; b.sub_shift = 3; CHECK(!halves_fit<C1>(b));          // the blocked layouts keep the whole-column kernel
  b = g; b.row_shift = 6; CHECK(!halves_fit<C1>(b));
  b = g; b.hi_shift = 4; CHECK(!halves_fit<C1>(b));
}
void test_halves() {
  CHECK(col_halves(0, 2048) == HALVES_OF_2048 && col_halves(0, 1024) == HALVES_OF_1024);
  CHECK((std::is_same<HalvesSel<HALVES_OF_2048>::type, GenSel<float, 1024>::type>::value));
  CHECK((std::is_same<HalvesSel<HALVES_OF_1024>::type, PairSel1024::type>::value));
  for (int N : {256, 512, 1023, 1025, 2047, 2049, 4096}) CHECK(col_halves(0, N) == HALVES_NONE);
  for (int N : {512, 1024, 2048, 4096}) CHECK(col_halves(1, N) == HALVES_NONE);          // float32 only
  test_fit<GenSel<float, 1024>::type>();
  test_fit<PairSel1024::type>();
  // the dispatching form: called with the served configuration when the geometry fits, not otherwise
  const ColGeom g{32, 32 * 1024, 32};
  int called = 0;
  CHECK(for_col_halves(0, 1024, g, [&](auto c) { called += std::is_same<typename decltype(c)::type, PairSel1024::type>::value; }) && called == 1);
  CHECK(for_col_halves(0, 2048, g, [&](auto c) { called += std::is_same<typename decltype(c)::type, GenSel<float, 1024>::type>::value; }) && called == 2);
  ColGeom blocked = g; blocked.sub_shift = 3;
  CHECK(!for_col_halves(0, 1024, blocked, [&](auto) { ++called; }) && !for_col_halves(1, 1024, g, [&](auto) { ++called; }) &&
        !for_col_halves(0, 512, g, [&](auto) { ++called; }) && called == 2);
}

// ---- fastgen_sequence: every tile exactly once, the kz = 0 tiles by the first launch -------------------------------------------------
struct Expect { int n; int kinds[3]; int ios[3]; };
void check_sequence(const char* what, const FastPass& c, int ny, int nzl, int kz0, bool full_rows, const Expect& want) {
  const long long ncols = (long long)ny * nzl, ntiles = ncols / c.tc, tiles_per_iy = nzl / c.tc;
  const ColGeom g{ncols, 0, ncols};
  const FastSequence q = fastgen_sequence(c, nzl, ncols, kz0, full_rows, g, true);
  CHECK(q.valid && q.n == want.n);
  if (!q.valid || q.n != want.n) { std::printf("  %s: valid=%d n=%d\n", what, (int)q.valid, q.n); return; }
  std::vector<int> seen(ntiles, 0), first(ntiles, 0);
  int records = 0;
  for (int i = 0; i < q.n; ++i) {
    const FastStep& st = q.step[i];
    CHECK(st.kind == want.kinds[i] && st.io == want.ios[i]);
    records += st.record_after;
    CHECK(!st.record_after || st.io == FAST_IO_FIRST);
    if (st.kind == FAST_FIX_FILL) { CHECK(i == 0 && c.side); continue; }
    CHECK(st.count > 0 && st.count < (1LL << 31));                     // a grid
    CHECK(st.skip_period == 0 || st.skip_period >= 2);                  // (the kernels divide by skip_period - 1)
    for (long long b = 0; b < st.count; ++b) {
      const long long t = fast_step_tile(st, b);
      for (long long u = (st.kind == FAST_COLPAIR ? 2 * t : t); u <= (st.kind == FAST_COLPAIR ? 2 * t + 1 : t); ++u) {
        CHECK(u >= 0 && u < ntiles);
        if (u < 0 || u >= ntiles) return;
        ++seen[u];
        first[u] |= st.io != FAST_IO_LEAN;
      }
    }
  }
  bool once = true, repaired = true;
  for (long long u = 0; u < ntiles; ++u) {
    once = once && seen[u] == 1;
    // the tile that holds slot kz = 0 of a ky row is run by a repairing kernel on the rank that owns kz = 0, and nowhere else is required
    if (kz0 == 0 && u % (tiles_per_iy > 0 ? tiles_per_iy : 1) == 0) repaired = repaired && first[u];
  }
  if (!once || !repaired) std::printf("  %s: once=%d repaired=%d\n", what, (int)once, (int)repaired);
  CHECK(once);
  CHECK(repaired);
  CHECK(records == (q.n >= 2 && kz0 == 0 ? 1 : 0));
  // without a side buffer the sequences that fill one are refused, the others unchanged
  const FastSequence nobuf = fastgen_sequence(c, nzl, ncols, kz0, full_rows, g, false);
  CHECK(nobuf.valid == (q.step[0].kind != FAST_FIX_FILL));
}
void test_sequences() {
  const int FF = FAST_FIX_FILL, C = FAST_COL, P = FAST_COLPAIR, C2 = FAST_COL2, L = FAST_IO_LEAN, R = FAST_IO_REPAIR, F = FAST_IO_FIRST;
  const FastPass h2048 = fast_pass_of<GenSel<float, 1024>::type>(true, 0), w1024 = fast_pass_of<GenSel<float, 1024>::type>(false, 0),
                 w1024n64 = fast_pass_of<GenSel<float, 1024>::type>(false, 1), h1024d = fast_pass_of<GenSel<double, 512>::type>(true, 0),
                 w64 = fast_pass_of<GenSel<float, 64>::type>(false, 0);
  CHECK(h2048.side && !h2048.pairs && w1024.side && w1024.pairs && !w1024n64.pairs && h1024d.side && !h1024d.pairs && !w64.side && !w64.pairs);
  CHECK(h2048.tc == 8 && w1024.tc == 8 && h1024d.tc == 8 && w64.tc == 32);
  for (int kz0 : {0, 16}) {
    const bool own = kz0 == 0;
    // N = 2048 float32, nzl = 8: a tile is a whole kz row, every tile repairs for itself
    check_sequence("2048 f32 nzl 8", h2048, 8, 8, kz0, true, {1, {C2}, {R}});
    // nzl = 16: split, halves
    check_sequence("2048 f32 nzl 16", h2048, 8, 16, kz0, true, own ? Expect{3, {FF, C2, C2}, {R, F, L}} : Expect{1, {C2}, {L}});
    // N = 1024 float32, nzl = 16: one pair per ky row, the first launch covers everything
    check_sequence("1024 f32 nzl 16", w1024, 8, 16, kz0, true, own ? Expect{2, {FF, P}, {R, F}} : Expect{1, {P}, {L}});
    // nzl = 32: two pairs per ky row
    check_sequence("1024 f32 nzl 32", w1024, 8, 32, kz0, true, own ? Expect{3, {FF, P, P}, {R, F, L}} : Expect{1, {P}, {L}});
    // the x slab of replicated generation, and resident float64 deviates: no pairs
    check_sequence("1024 f32 slab", w1024, 8, 32, kz0, false, own ? Expect{3, {FF, C, C}, {R, F, L}} : Expect{1, {C}, {L}});
    check_sequence("1024 f32 noise64", w1024n64, 8, 32, kz0, true, own ? Expect{3, {FF, C, C}, {R, F, L}} : Expect{1, {C}, {L}});
    // N = 1024 float64, nzl = 16: halves
    check_sequence("1024 f64 nzl 16", h1024d, 8, 16, kz0, true, own ? Expect{3, {FF, C2, C2}, {R, F, L}} : Expect{1, {C2}, {L}});
    // N = 64: short pass, the owning lane repairs (no side buffer); tiles of 32 columns, so nzl = 64 splits and nzl = 32 does not
    check_sequence("64 f32 nzl 64", w64, 32, 64, kz0, true, own ? Expect{2, {C, C}, {F, L}} : Expect{1, {C}, {L}});
    check_sequence("64 f32 nzl 32", w64, 32, 32, kz0, true, {1, {C}, {R}});
  }
  // pairs need whole pairs per kz row and per run of `inner` columns, and the plain layout: else single tiles
  ColGeom blocked{8 * 32, 0, 8 * 32};
  blocked.sub_shift = 3;
  const FastSequence q = fastgen_sequence(w1024, 32, 8 * 32, 0, true, blocked, true);
  CHECK(q.valid && q.n == 3 && q.step[1].kind == FAST_COL && q.step[2].kind == FAST_COL);
  const FastSequence q3 = fastgen_sequence(w1024, 24, 8 * 24, 0, true, ColGeom{8 * 24, 0, 8 * 24}, true);      // 3 tiles per kz row
  CHECK(q3.valid && q3.n == 3 && q3.step[1].kind == FAST_COL);
}

// ---- yz_slabs: the partition of the nx planes for the y / z passes --------------------------------------------------------------------
bool same(const YzSlabs& a, int planes, int count, int last) { return a.planes == planes && a.count == count && a.last == last; }
void test_slabs() {
  CHECK(same(yz_slabs(256, 64, false, 0), 64, 4, 64));          // a size that divides nx
  CHECK(same(yz_slabs(8, 3, false, 0), 3, 3, 2));               // ... and one that does not: a smaller last slab
  CHECK(same(yz_slabs(256, 48, false, 0), 48, 6, 16));
  CHECK(same(yz_slabs(8, 8, false, 0), 8, 1, 8));               // a size >= nx: one slab
  CHECK(same(yz_slabs(8, 100, false, 0), 8, 1, 8));
  CHECK(same(yz_slabs(8, 0, false, 0), 8, 1, 8));               // whole-grid passes asked for, or automatic and nothing to gain
  CHECK(same(yz_slabs(8, -1, false, 0), 8, 1, 8));
  CHECK(same(yz_slabs(8, 1, false, 0), 1, 8, 1));
  // the blocked intermediate: whole row blocks, a power of two of them, dividing nx -- else one slab
  CHECK(same(yz_slabs(256, 64, true, 16), 64, 4, 64));
  CHECK(same(yz_slabs(256, 16, true, 16), 16, 16, 16));
  CHECK(same(yz_slabs(256, 24, true, 16), 256, 1, 256));        // not whole row blocks
  CHECK(same(yz_slabs(256, 48, true, 16), 256, 1, 256));        // whole row blocks, not a power of two
  CHECK(same(yz_slabs(192, 128, true, 16), 192, 1, 192));       // a power of two of row blocks that does not divide nx
  CHECK(same(yz_slabs(192, 64, true, 16), 64, 3, 64));
  CHECK(same(yz_slabs(256, 0, true, 16), 256, 1, 256));
  CHECK(same(yz_slabs(192, 128, false, 16), 128, 2, 64));       // (the plain layout takes any size)
}

}  // namespace

int main() {
  test_variants();
  test_halves();
  test_sequences();
  test_slabs();
  if (g_failed) { std::printf("%d of %d checks FAILED\n", g_failed, g_checked); return 1; }
  std::printf("all checks passed (%d)\n", g_checked);
  return 0;
}
