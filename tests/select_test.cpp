// select_test.cpp -- the pure host functions that choose the tiled kernels (randomfield_amd/csrc/rf_select.h): which fast generation
// variant, which pass runs as Col2 halves, which launches a fast generation pass makes, and the shapes each pass can serve (tile widths,
// row blocks, the gathering z pass, the blocked intermediate, direct stores, replicated generation).  Stand-alone: compiled with
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

// ---- the shapes a pass can serve: literal tables ----------------------------------------------------------------------------------------
void test_shapes() {
  const int N[9] = {8, 16, 32, 64, 128, 256, 512, 1024, 2048};
  // tile widths: the in-place pass and the generating x pass use the same tiles at every length
  const int tc[2][9] = {{32, 32, 32, 32, 32, 16, 16, 8, 8}, {16, 16, 16, 16, 16, 8, 8, 8, 4}};
  // x rows per block of the blocked intermediate for want = 16 and 64 (0 and N: no blocking): `want` where the last pass's row offsets
  // N / RL are whole blocks.  One-pass lengths (8, 16) never block; float64 1024 has RL = 16, so N / RL = 64
  const int rb16[2][9] = {{8, 16, 32, 64, 16, 16, 16, 16, 16}, {8, 16, 32, 64, 16, 16, 16, 16, 16}};
  const int rb64[2][9] = {{8, 16, 32, 64, 128, 256, 64, 64, 64}, {8, 16, 32, 64, 128, 256, 64, 64, 64}};
  for (int f64 = 0; f64 < 2; ++f64)
    for (int i = 0; i < 9; ++i) {
      CHECK(col_tile_cols(f64, N[i]) == tc[f64][i] && col_gen_tile_cols(f64, N[i]) == tc[f64][i]);
      CHECK(col_gen_row_block(f64, N[i], 0) == N[i] && col_gen_row_block(f64, N[i], N[i]) == N[i]);
      CHECK(col_gen_row_block(f64, N[i], 16) == rb16[f64][i]);
      CHECK(col_gen_row_block(f64, N[i], 64) == rb64[f64][i]);
      CHECK(col_gen_row_block(f64, N[i], 24) == N[i]);                   // not a power of two
    }
  for (int f64 = 0; f64 < 2; ++f64)
    for (int n : {0, 4, 100, 4096}) CHECK(col_tile_cols(f64, n) == 0 && col_gen_tile_cols(f64, n) == 0 && col_gen_row_block(f64, n, 16) == n);
  // the gathering z pass: x blocks of whole workgroups (rb a multiple of NRT: 8 rows at M = 512 float32, 64 at M = 32, float64 64 at M = 16
  // and 2 at M = 1024), whole tiles per row
  struct { int f64, M, tc, rb; bool ok; } xg[] = {{0, 512, 8, 64, true}, {0, 512, 8, 8, true}, {0, 512, 8, 4, false}, {0, 32, 32, 64, true},
      {0, 32, 32, 32, false}, {1, 16, 16, 32, false}, {1, 16, 16, 64, true}, {1, 1024, 8, 2, true}, {1, 1024, 8, 1, false}, {0, 512, 0, 64, false},
      {0, 512, 8, 0, false}, {0, 512, 24, 64, false}, {0, 100, 4, 64, false}, {0, 2048, 8, 64, false}};
  for (const auto& c : xg) CHECK(row_c2r_xgather_ok(c.f64, c.M, c.tc, c.rb) == c.ok);
  CHECK(row_c2r_tiles(0, 512, 17) == 3 && row_c2r_tiles(1, 512, 17) == 5 && row_c2r_tiles(0, 8, 256) == 1 && row_c2r_tiles(0, 8, 257) == 2 &&
        row_c2r_tiles(0, 100, 5) == -1);
  // the blocked intermediate (nx, ny, nzl, nzc, row block): x and y tiles of one width, kz runs of whole tiles, a z pass that can gather
  auto xp = [](int f64, int nx, int ny, long long nzl, long long nzc) { return xpose_shape_ok(f64, nx, ny, nzl, nzc, col_gen_row_block(f64, nx, 64)); };
  CHECK(xp(0, 64, 64, 32, 32) && xp(0, 128, 64, 32, 32) && xp(0, 1024, 1024, 32, 32) && xp(1, 64, 64, 64, 64) && xp(0, 512, 512, 32, 32));
  CHECK(!xp(0, 512, 16, 32, 32));                   // x tiles of 16 columns, y tiles of 32
  CHECK(!xp(1, 32, 32, 16, 16));                    // 32 x rows per block, 64 rows per workgroup of the z pass
  CHECK(!xp(0, 64, 64, 16, 16));                    // a kz run narrower than a tile
  CHECK(!xp(0, 1024, 1024, 12, 32));                // ... and one of one and a half tiles
  CHECK(!xp(0, 100, 64, 32, 32) && !xp(0, 64, 100, 32, 32) && !xp(0, 64, 64, 32, 100));
  // direct stores: whole tiles per x plane (inner a power of two, a multiple of the tile width)
  struct { int f64, N; long long inner; bool ok; } dr[] = {{0, 1024, 8, true}, {0, 1024, 4, false}, {0, 1024, 24, false}, {0, 1024, 16, true},
      {0, 64, 32, true}, {0, 64, 16, false}, {0, 100, 64, false}, {0, 64, 0, false}, {0, 64, -32, false}, {1, 2048, 4, true}, {1, 2048, 2, false}};
  for (const auto& c : dr) CHECK(col_direct_supported(c.f64, c.N, c.inner) == c.ok);
  // replicated generation: a fast pass with an LDS stage whose slabs N / nranks are multiples of N / RL, i.e. nranks divides RL (8 at 64,
  // 512, 1024; 4 at 32; 16 at 2048)
  struct { int f64, N, nranks; bool ok; } rp[] = {{0, 1024, 1, true}, {0, 1024, 8, true}, {0, 1024, 16, false}, {0, 1024, 3, false}, {0, 1024, 0, false},
      {0, 16, 1, false}, {0, 8, 2, false}, {0, 64, 8, true}, {0, 64, 16, false}, {0, 32, 4, true}, {0, 32, 8, false}, {0, 2048, 16, true},
      {0, 2048, 32, false}, {1, 2048, 2, false}, {1, 1024, 8, true}, {0, 100, 2, false}};
  for (const auto& c : rp) CHECK(col_replicate_supported(c.f64, c.N, c.nranks) == c.ok);
  CHECK(col_fastgen_supported(0, 2048) && !col_fastgen_supported(1, 2048) && col_fastgen_supported(1, 1024) && !col_fastgen_supported(0, 100));
  // 64-bit lane offsets exist from length 1024 on
  const ColGeom small{64, 64 * 8, 64}, huge{1LL << 30, 0, 1LL << 30};
  for (int f64 = 0; f64 < 2; ++f64) {
    for (int n : N) CHECK(col_plain_addressable(f64, n, small) && col_plain_addressable(f64, n, huge) == (n >= 1024 || n == 8 || n == 16));
    CHECK(!col_plain_addressable(f64, 100, small));
  }
  // the lognormal z pass keeps its exp table in spare LDS slots for float64 rows of >= 512 complex
  CHECK((std::is_same<LognormalIO<double, 512>, LognormalRowIO<double, 1>>::value && std::is_same<LognormalIO<double, 1024>, LognormalRowIO<double, 1>>::value));
  CHECK((std::is_same<LognormalIO<double, 256>, LognormalRowIO<double, 0>>::value && std::is_same<LognormalIO<float, 1024>, LognormalRowIO<float, 0>>::value));
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
  test_shapes();
  test_slabs();
  if (g_failed) { std::printf("%d of %d checks FAILED\n", g_failed, g_checked); return 1; }
  std::printf("all checks passed (%d)\n", g_checked);
  return 0;
}
