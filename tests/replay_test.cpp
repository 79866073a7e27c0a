// replay_test.cpp -- the host side of the MT19937 replay (randomfield_amd/csrc/rf_replay.h) against the code it replaced.  The functions
// of namespace old below are LITERAL COPIES of what rf_capi_mt.hip held inside its HIP entry points before the change -- mt_geom, the
// jump-tree loops of mt_queue and of rf_mt_share_begin, the digit hop of rf_mt_share_begin, the split of rf_mt_share_pack, the widening of
// rf_mt_set_jump, the `sh_state` comparisons of the six share calls -- over a struct that has the plan's members of those names, with the
// HIP calls taken out (a launch is recorded instead of made).  Every function of the header is compared with its copy over the ranges
// listed at each section, and the tree and the split are held to invariants of their own.  Stand-alone: compiled with
// -fsanitize=address,undefined and run by tests/test_replay_plan.py; exit status 0 = every check held.
//
//   replay_test                      all checks
//   replay_test geom nx ny nz bps    prints "nseg stages last_nb cap" of that grid's replay at radix 16
//   replay_test split nseg nranks    prints the ranks' first segments
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../randomfield_amd/csrc/rf_replay.h"

namespace {

long long g_failed = 0, g_checks = 0;
char g_where[200];
#define CHECK(cond)                                                              \
  do {                                                                           \
    ++g_checks;                                                                  \
    if (!(cond)) { if (g_failed < 50) std::printf("FAILED %s:%d: %s   [%s]\n", __FILE__, __LINE__, #cond, g_where); ++g_failed; } \
  } while (0)

// the text of the last refusal of an old function (RF_REQUIRE: `return fail(1, msg)`)
const char* g_old_text = nullptr;
int fail(int code, const char* msg) { g_old_text = msg; return code; }
#define RF_REQUIRE(cond, msg) \
  do {                        \
    if (!(cond)) return fail(1, msg); \
  } while (0)
bool same_text(const char* a, const char* b) { return (a == nullptr) == (b == nullptr) && (!a || std::strcmp(a, b) == 0); }

// a fixed linear congruential generator (Knuth's MMIX constants), high bits
struct Lcg {
  unsigned long long s;
  explicit Lcg(unsigned long long seed) : s(seed) {}
  unsigned next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (unsigned)(s >> 33); }
};

// the plan members the old expressions read
struct Plan {
  int nx = 1, ny = 1, nzc = 0, nzl = 0, nranks = 1, rank = 0;
  std::vector<int> mt_npos;
  int mt_bps = 1, mt_radix = 16;
  int sh_state = 0;
  int sh_single = 0;
  unsigned long long sh_total = 0;
  std::vector<unsigned long long> sh_sendoff, sh_sendcnt, sh_recvoff, sh_recvcnt;
};

// one recorded launch of the jump kernel: first row of the table, sources, distance, multipliers, segment bound
struct Jump {
  int row, nsrc;
  long long dist;
  int nmul, nseg;
  bool operator==(const Jump& o) const { return row == o.row && nsrc == o.nsrc && dist == o.dist && nmul == o.nmul && nseg == o.nseg; }
};

namespace old {
// rf_capi_mt.hip MtGeom / mt_geom
struct MtGeom {
  unsigned long long ncells, attempts, cap;
  long long total_blocks;
  int nseg, stages;
  size_t need;          // bytes of the runs: nseg * cap pairs
};
int mt_geom(Plan* p, int single, MtGeom& g) {
  g.ncells = (unsigned long long)p->nx * p->ny * (p->nzc + 1);
  // polar attempts to generate: acceptance pi/4, margin of 10 sigma + 1024 (mt19937.attempts_needed)
  const double pa = 0.78539816339744830962;
  g.attempts = (unsigned long long)std::ceil((double)g.ncells / pa + 10.0 * std::sqrt((double)g.ncells * (1 - pa)) / pa + 1024.0);
  g.total_blocks = (long long)((4 * g.attempts + 623) / 624);
  g.nseg = (int)((g.total_blocks + p->mt_bps - 1) / p->mt_bps);
  // stages of the radix-R jump tree: stage t needs the R - 1 polynomials t^(m R^t L), rows t (R - 1) .. of the table
  const int R = p->mt_radix;
  g.stages = 0;
  long long reach = 1;
  while (reach < g.nseg) { reach *= R; ++g.stages; }
  RF_REQUIRE(g.stages * (R - 1) <= (int)p->mt_npos.size(), "grid too large for the uploaded jump table");
  g.cap = (unsigned long long)p->mt_bps * (624 / 4);
  g.need = (size_t)g.nseg * g.cap * (single ? 2 * sizeof(float) : 2 * sizeof(double));
  return 0;
}
bool pairs32_fit(const Plan* p, const MtGeom& g) { return g.cap >= 4ull * (unsigned long long)(p->nzc + 1); }

// rf_capi_mt.hip mt_queue: the jump tree (launch_mt_jump(states, pos + t (R - 1) stride, npos_dev + 4 t (R - 1), stride, nsrc, dist, R - 1, g.nseg, s))
void mt_queue_tree(const Plan* p, const MtGeom& g, std::vector<Jump>& out) {
  const int R = p->mt_radix;
  long long dist = 1;
  for (int t = 0; t < g.stages; ++t, dist *= R) {
    const int nsrc = (int)(dist < g.nseg ? dist : g.nseg);
    out.push_back(Jump{t * (R - 1), nsrc, dist, R - 1, g.nseg});
  }
}
// rf_capi_mt.hip rf_mt_share_begin: the local tree ("mt_queue with a shifted origin")
void share_begin_tree(const Plan* p, int nloc, std::vector<Jump>& out) {
  const int R = p->mt_radix;
  long long dist = 1;
  for (int t = 0; dist < nloc; ++t, dist *= R) {
    const int nsrc = (int)(dist < nloc ? dist : nloc);
    out.push_back(Jump{t * (R - 1), nsrc, dist, R - 1, nloc});
  }
}
// rf_capi_mt.hip rf_mt_share_begin: the hop to segment `first` (launch_mt_jump(states + slot 624, pos + row stride, npos_dev + 4 row, stride, 1, 1, 1, 2, s))
int share_begin_hops(const Plan* p, const MtGeom& g, int first, int nloc, std::vector<int>& rows, int& slot_out) {
  const int R = p->mt_radix;
  int slot = nloc;
  {
    int rest = first;
    for (int t = 0; rest > 0; ++t, rest /= R) {
      const int d = rest % R;
      if (d == 0) continue;
      RF_REQUIRE(t < g.stages && slot + 1 < nloc + 8, "segment index beyond the uploaded jump table");
      const int row = t * (R - 1) + d - 1;
      rows.push_back(row);
      ++slot;
    }
  }
  slot_out = slot;
  return 0;
}

inline int sh_seg_begin(int r, int nseg, int nranks) { return (int)((long long)r * nseg / nranks); }

// rf_capi_mt.hip rf_mt_share_pack, from behind mt_geom to the first buffer: off and sbase were locals
int share_pack(Plan* p, const MtGeom& g, const unsigned long long* counts_all, std::vector<unsigned long long>& off, std::vector<long long>& sbase) {
  const int P = p->nranks, nzl = (int)p->nzl, nzh = (int)p->nzc + 1;
  off.assign((size_t)g.nseg + 1, 0);
  off[0] = 0;
  for (int i = 0; i < g.nseg; ++i) {
    RF_REQUIRE(counts_all[i] <= g.cap, "a segment cannot hold more pairs than attempts: the gathered counts are corrupt");
    off[i + 1] = off[i] + counts_all[i];
  }
  RF_REQUIRE(off[g.nseg] >= g.ncells, "MT19937 replay: not enough accepted polar attempts (increase the margin)");
  p->sh_total = off[g.nseg];
  // first cell of every rank's share, and the index in "stream q" (rows of nzl + 1 pairs: q's planes, then the Nyquist plane) of
  // the first stream-q cell at or behind stream cell c
  std::vector<unsigned long long> cb((size_t)P + 1);
  for (int r = 0; r <= P; ++r) {
    const unsigned long long c = off[sh_seg_begin(r, g.nseg, P)];
    cb[r] = c < g.ncells ? c : g.ncells;
  }
  cb[P] = g.ncells;
  auto fq = [&](int q, unsigned long long c) -> unsigned long long {
    const unsigned long long col = c / (unsigned)nzh;
    long long k = (long long)(c - col * (unsigned)nzh) - (long long)q * nzl;
    k = k < 0 ? 0 : (k > nzl ? nzl : k);
    return col * (unsigned)(nzl + 1) + (unsigned long long)k;
  };
  const int me = p->rank;
  p->sh_sendoff.assign(P + 1, 0); p->sh_sendcnt.assign(P, 0); p->sh_recvoff.assign(P, 0); p->sh_recvcnt.assign(P, 0);
  sbase.assign(P, 0);
  for (int q = 0; q < P; ++q) {
    p->sh_sendcnt[q] = fq(q, cb[me + 1]) - fq(q, cb[me]);
    p->sh_sendoff[q + 1] = p->sh_sendoff[q] + p->sh_sendcnt[q];
    sbase[q] = (long long)p->sh_sendoff[q] - (long long)fq(q, cb[me]);
    p->sh_recvoff[q] = fq(me, cb[q]);                     // (q = the sending rank here)
    p->sh_recvcnt[q] = fq(me, cb[q + 1]) - fq(me, cb[q]);
  }
  return 0;
}

// rf_capi_mt.hip rf_mt_set_jump, between the release of the old table and the upload
int set_jump_widen(int npolys, const uint16_t* pos, const int* npos, int stride, std::vector<uint32_t>& wide, std::vector<int>& counts, int& wstride_out) {
  const uint32_t null_off = 4u * 33u * 624u;
  const int wstride = ((stride + 7) / 8 + 4) * 8;
  wide.assign((size_t)npolys * wstride, null_off);
  counts.assign(4 * (size_t)npolys, 0);
  wstride_out = wstride;
  for (int l = 0; l < npolys; ++l) {
    int n[4] = {0, 0, 0, 0};
    for (int j = 0; j < npos[l]; ++j) ++n[pos[(size_t)l * stride + j] & 3];
    int off[4], padded[4];
    for (int c = 0, o = 0; c < 4; ++c) { padded[c] = (n[c] + 7) & ~7; off[c] = o; o += padded[c]; }
    RF_REQUIRE(off[3] + padded[3] <= wstride, "jump table row too long");
    int k[4] = {0, 0, 0, 0};
    for (int j = 0; j < npos[l]; ++j) {
      const uint32_t q = pos[(size_t)l * stride + j];
      const int c = (int)(q & 3u);
      wide[(size_t)l * wstride + off[c] + k[c]++] = 4u * (q - (uint32_t)c);
    }
    for (int c = 0; c < 4; ++c) counts[4 * l + c] = padded[c];
  }
  return 0;
}

// rf_capi_mt.hip rf_mt_share_exchange_local as far as it reads and writes sh_state
int share_exchange_local(Plan** plans, int n) {
  for (int g = 0; g < n; ++g)
    RF_REQUIRE(plans[g]->sh_state == 2 && plans[g]->sh_single == plans[0]->sh_single, "rf_mt_share_pack must have run on every plan (same mode)");
  for (int g = 0; g < n; ++g) plans[g]->sh_state = 3;
  return 0;
}
// the six share calls as far as they read and write sh_state (a call that gets past its check succeeds, but for BEGIN_FAILS: a
// rf_mt_share_begin that fails behind `p->sh_state = 0`); the local exchange is given the plan itself as its one rank
enum Call { BEGIN, BEGIN_FAILS, GATHER, PACK, EXCHANGE, EXCHANGE_LOCAL, FINISH, NCALLS };
int share_call(Plan* p, Call c, int single) {
  switch (c) {
    case BEGIN: p->sh_state = 0; p->sh_single = single; p->sh_state = 1; return 0;
    case BEGIN_FAILS: p->sh_state = 0; return fail(2, "hip");
    case GATHER: RF_REQUIRE(p->sh_state == 1, "rf_mt_share_begin must be called first"); return 0;
    case PACK: RF_REQUIRE(p->sh_state == 1, "rf_mt_share_begin must be called first"); p->sh_state = 2; return 0;
    case EXCHANGE: RF_REQUIRE(p->sh_state == 2, "rf_mt_share_pack must be called first"); p->sh_state = 3; return 0;
    case EXCHANGE_LOCAL: return share_exchange_local(&p, 1);
    case FINISH: RF_REQUIRE(p->sh_state == 3, "the exchange must have run first"); p->sh_state = 0; return 0;
    default: return -1;
  }
}
}  // namespace old

// the same calls on the step type, as rf_capi_mt.hip makes them now
const char* g_new_text = nullptr;
int share_call(rfc::ShareStep& st, old::Call c, bool single) {
  auto refuse = [](const char* why) { g_new_text = why; return 1; };
  switch (c) {
    case old::BEGIN: st.reset(); st.replay_done(single); return 0;
    case old::BEGIN_FAILS: st.reset(); g_new_text = "hip"; return 2;
    case old::GATHER: if (const char* why = st.refuses_gather()) return refuse(why); return 0;
    case old::PACK: if (const char* why = st.refuses_pack()) return refuse(why); st.pack_done(); return 0;
    case old::EXCHANGE: if (const char* why = st.refuses_exchange()) return refuse(why); st.exchange_done(); return 0;
    case old::EXCHANGE_LOCAL: if (const char* why = st.refuses_exchange_local(st)) return refuse(why); st.exchange_done(); return 0;
    case old::FINISH: if (const char* why = st.refuses_finish()) return refuse(why); st.finish_done(); return 0;
    default: return -1;
  }
}

// ---- geometry: every ncells in 1 .. 70 000 and those of 1024^3 and 2048^3, bps in {1, 2, 3, 16, 107, 8192}, radix in {2, 16}, single in {0, 1}
void check_geom_one(int nx, int ny, int nzc) {
  const int bpss[] = {1, 2, 3, 16, 107, 8192}, radices[] = {2, 16};
  for (int bps : bpss)
    for (int radix : radices)
      for (int single = 0; single < 2; ++single) {
        std::snprintf(g_where, sizeof(g_where), "geom nx=%d ny=%d nzc=%d bps=%d radix=%d single=%d", nx, ny, nzc, bps, radix, single);
        Plan p;
        p.nx = nx; p.ny = ny; p.nzc = nzc; p.mt_bps = bps; p.mt_radix = radix;
        const rfc::ReplayGeom g = rfc::replay_geom((unsigned long long)nx * ny * (nzc + 1), bps, radix, single != 0);
        CHECK(g.stages == rfc::tree_stages(g.nseg, radix));
        // the table: exactly the rows the grid needs, and one row short
        rfc::JumpTable tab;
        tab.bps = bps; tab.radix = radix;
        for (int less = 0; less < 2; ++less) {
          const int rows = g.stages * (radix - 1) - less;
          if (rows < 0) continue;
          p.mt_npos.assign((size_t)rows, 1);
          tab.npos = p.mt_npos;
          old::MtGeom o;
          g_old_text = nullptr;
          const int rc = old::mt_geom(&p, single, o);
          CHECK(rc == (less ? 1 : 0));
          CHECK(same_text(rc ? g_old_text : nullptr, tab.refuses(g)));
          if (rc) continue;
          CHECK(g.ncells == o.ncells && g.attempts == o.attempts && g.cap == o.cap && g.total_blocks == o.total_blocks);
          CHECK(g.nseg == o.nseg && g.stages == o.stages && g.need == o.need);
          CHECK(rfc::pairs32_fit(g, nzc + 1) == old::pairs32_fit(&p, o));
        }
      }
}
void check_geom() {
  for (int n = 1; n <= 70000; ++n) check_geom_one(1, 1, n - 1);
  check_geom_one(1024, 1024, 512);
  check_geom_one(2048, 2048, 1024);
}

// ---- the tree: nseg in 1 .. 70 000 at radix 16 (across 16^4), 1 .. 4097 at radix 2
std::vector<Jump> new_tree(int nseg, int radix) {
  std::vector<Jump> out;
  const int rc = rfc::for_each_tree_stage(nseg, radix, [&](int t, int nsrc, long long dist) {
    out.push_back(Jump{t * (radix - 1), nsrc, dist, radix - 1, nseg});
    return 0;
  });
  CHECK(rc == 0);
  return out;
}
void check_tree(int radix, int nseg_max) {
  std::vector<int> hit;
  for (int nseg = 1; nseg <= nseg_max; ++nseg) {
    std::snprintf(g_where, sizeof(g_where), "tree radix=%d nseg=%d", radix, nseg);
    Plan p;
    p.mt_radix = radix;
    old::MtGeom g{};
    g.nseg = nseg;
    {                                               // old::mt_geom's stage count, literally
      const int R = p.mt_radix;
      g.stages = 0;
      long long reach = 1;
      while (reach < g.nseg) { reach *= R; ++g.stages; }
    }
    CHECK(g.stages == rfc::tree_stages(nseg, radix));
    std::vector<Jump> a, b;
    old::mt_queue_tree(&p, g, a);
    old::share_begin_tree(&p, nseg, b);
    const std::vector<Jump> n = new_tree(nseg, radix);
    CHECK(n == a);
    CHECK(n == b);
    CHECK((int)n.size() == g.stages);
    if (nseg > 5000) continue;
    // every segment 1 .. nseg - 1 is the destination src + m dist of exactly one (stage, source, multiplier), none is >= nseg when
    // the kernel's bound (its last argument) is applied, and a source is a state that an earlier stage (or the start) has made
    hit.assign((size_t)nseg, 0);
    hit[0] = 1;
    bool ordered = true;
    for (const Jump& j : n)
      for (int m = 1; m <= j.nmul; ++m)
        for (int src = 0; src < j.nsrc; ++src) {
          const long long dst = src + m * j.dist;
          if (dst >= j.nseg) continue;
          if (!hit[(size_t)src]) ordered = false;
          ++hit[(size_t)dst];
        }
    bool once = true;
    for (int s = 0; s < nseg; ++s) once = once && hit[(size_t)s] == 1;
    CHECK(once);
    CHECK(ordered);
  }
  // a walk that is told to stop stops, and hands the code back
  int calls = 0;
  CHECK(rfc::for_each_tree_stage(70000, 16, [&](int, int, long long) { return ++calls == 2 ? 7 : 0; }) == 7 && calls == 2);
}

// ---- the hops: first in 0 .. 70 000 at radix 16 (and 0 .. 4097 at radix 2, where eight non-zero digits are common), every stage count 0 .. 4 (0 .. 13)
void check_hops(int radix, int first_max, int stages_max) {
  for (int first = 0; first <= first_max; ++first)
    for (int stages = 0; stages <= stages_max; ++stages) {
      std::snprintf(g_where, sizeof(g_where), "hops radix=%d first=%d stages=%d", radix, first, stages);
      Plan p;
      p.mt_radix = radix;
      old::MtGeom g{};
      g.stages = stages;
      const int nloc = 1 + first % 5;
      std::vector<int> rows;
      int slot = 0;
      g_old_text = nullptr;
      const int rc = old::share_begin_hops(&p, g, first, nloc, rows, slot);
      const rfc::Hops h = rfc::digit_hops(first, radix, stages);
      CHECK(same_text(rc ? g_old_text : nullptr, h.refusal));
      if (rc) continue;
      CHECK(h.n == (int)rows.size() && nloc + h.n == slot && nloc + h.n < nloc + rfc::kSpareSlots);
      bool same = h.n == (int)rows.size();
      for (int i = 0; same && i < h.n; ++i) same = h.rows[i] == rows[(size_t)i];
      CHECK(same);
    }
}

// ---- the split: nranks in {1, 2, 3, 4, 8, 64}, nx ny in {1, 4, 64}, nzl in {2, 4, 16}, nzh = nranks nzl + 1, counts from the LCG
// mode 0: counts <= cap that suffice; 1: one count above cap; 2: a total below ncells
void check_split_case(int nranks, int nxny, int nzl, int mode) {
  Plan p;
  p.nx = nxny; p.ny = 1; p.nzl = nzl; p.nzc = nranks * nzl; p.nranks = nranks; p.mt_bps = 1; p.mt_radix = 16;
  p.mt_npos.assign(60, 1);
  const int nzh = p.nzc + 1;
  old::MtGeom o;
  if (old::mt_geom(&p, 1, o)) { CHECK(false); return; }
  const rfc::ReplayGeom g = rfc::replay_geom((unsigned long long)nxny * nzh, 1, 16, true);
  Lcg lcg(1000003ull * nranks + 1009ull * nxny + nzl);
  std::vector<unsigned long long> counts((size_t)o.nseg);
  // (just enough pairs: the last ranks' shares end inside the cells, as the real stream's do on a large grid)
  const unsigned long long base = o.ncells / (unsigned)o.nseg + 1;
  for (auto& c : counts) {
    c = mode == 2 ? lcg.next() % 2 : base + lcg.next() % 8;
    if (c > o.cap) c = o.cap;
  }
  if (mode == 1) counts[(size_t)(lcg.next() % (unsigned)o.nseg)] = o.cap + 1;
  std::vector<rfc::ShareSplit> all;
  for (int r = 0; r < nranks; ++r) {
    std::snprintf(g_where, sizeof(g_where), "split nranks=%d nxny=%d nzl=%d mode=%d rank=%d nseg=%d", nranks, nxny, nzl, mode, r, o.nseg);
    p.rank = r;
    std::vector<unsigned long long> off;
    std::vector<long long> sbase;
    g_old_text = nullptr;
    const int rc = old::share_pack(&p, o, counts.data(), off, sbase);
    rfc::ShareSplit s = rfc::share_split(counts.data(), g, nranks, r, nzl, nzh);
    CHECK(rc == (mode ? 1 : 0));
    CHECK(same_text(rc ? g_old_text : nullptr, s.refusal));
    if (rc) continue;
    CHECK(s.first == off && s.total == p.sh_total && s.sbase == sbase);
    CHECK(s.sendoff == p.sh_sendoff && s.sendcnt == p.sh_sendcnt && s.recvoff == p.sh_recvoff && s.recvcnt == p.sh_recvcnt);
    CHECK(rfc::sh_seg_begin(r, o.nseg, nranks) == old::sh_seg_begin(r, o.nseg, nranks));
    all.push_back(std::move(s));
  }
  if (mode) return;
  // across ranks
  const unsigned long long per_rank = (unsigned long long)nxny * (nzl + 1);
  for (int g0 = 0; g0 < nranks; ++g0) {
    std::snprintf(g_where, sizeof(g_where), "split invariants nranks=%d nxny=%d nzl=%d rank=%d", nranks, nxny, nzl, g0);
    const rfc::ShareSplit& s = all[(size_t)g0];
    bool mirrored = true, tiled = s.recvoff[0] == 0;
    unsigned long long sent = 0;
    for (int h = 0; h < nranks; ++h) {
      mirrored = mirrored && s.sendcnt[(size_t)h] == all[(size_t)h].recvcnt[(size_t)g0];
      const unsigned long long end = s.recvoff[(size_t)h] + s.recvcnt[(size_t)h];
      tiled = tiled && end == (h + 1 < nranks ? s.recvoff[(size_t)h + 1] : per_rank);
      sent += s.sendcnt[(size_t)h];
    }
    CHECK(mirrored);       // what g sends to h is what h expects from g
    CHECK(tiled);          // the receive ranges tile [0, nx ny (nzl + 1)) without gap or overlap
    // the sends of rank g are the cells of its share of the stream: cells [a, b) of the first ncells, each to the rank that owns its
    // plane -- and a cell of the Nyquist plane (c mod nzh == nzh - 1; floor(x / nzh) of them below x) to every rank
    const unsigned long long nc = g.ncells;
    unsigned long long a = s.first[(size_t)rfc::sh_seg_begin(g0, g.nseg, nranks)], b = s.first[(size_t)rfc::sh_seg_begin(g0 + 1, g.nseg, nranks)];
    a = a < nc ? a : nc;
    b = g0 + 1 == nranks || b > nc ? nc : b;
    CHECK(sent == (b - a) + (unsigned long long)(nranks - 1) * (b / (unsigned)nzh - a / (unsigned)nzh));
    CHECK(s.sendoff[(size_t)nranks] == sent);
  }
}
void check_split() {
  const int ranks[] = {1, 2, 3, 4, 8, 64}, planes[] = {1, 4, 64}, nzls[] = {2, 4, 16};
  for (int nranks : ranks)
    for (int nxny : planes)
      for (int nzl : nzls) check_split_case(nranks, nxny, nzl, 0);
  check_split_case(4, 64, 4, 1);
  check_split_case(4, 64, 4, 2);
}

// ---- the step: every sequence of the calls up to length five, against the integer
void check_step() {
  for (int len = 1; len <= 5; ++len) {
    int total = 1;
    for (int i = 0; i < len; ++i) total *= old::NCALLS;
    for (int code = 0; code < total; ++code) {
      Plan p;
      rfc::ShareStep st;
      int c = code;
      for (int i = 0; i < len; ++i, c /= old::NCALLS) {
        const old::Call call = (old::Call)(c % old::NCALLS);
        const int single = (code + i) & 1;
        std::snprintf(g_where, sizeof(g_where), "step sequence %d of length %d, call %d = %d", code, len, i, (int)call);
        g_old_text = g_new_text = nullptr;
        const int ro = old::share_call(&p, call, single), rn = share_call(st, call, single != 0);
        CHECK(ro == rn);
        CHECK(same_text(ro ? g_old_text : nullptr, rn ? g_new_text : nullptr));
        CHECK((p.sh_state == 0) == st.idle() && (p.sh_state == 1) == st.replayed() && (p.sh_state == 2) == st.packed() && (p.sh_state == 3) == st.exchanged());
        CHECK((p.sh_single != 0) == st.single());
      }
    }
  }
  // the local exchange between plans of two modes: `plans[g]->sh_state == 2 && plans[g]->sh_single == plans[0]->sh_single`
  for (int s0 = 0; s0 < 2; ++s0)
    for (int s1 = 0; s1 < 2; ++s1)
      for (int packed = 0; packed < 2; ++packed) {
        std::snprintf(g_where, sizeof(g_where), "local exchange modes %d %d packed %d", s0, s1, packed);
        Plan p0, p1;
        p0.sh_state = 2; p0.sh_single = s0;
        p1.sh_state = packed ? 2 : 1; p1.sh_single = s1;
        Plan* plans[2] = {&p0, &p1};
        rfc::ShareStep a, b;
        a.replay_done(s0 != 0); a.pack_done();
        b.replay_done(s1 != 0);
        if (packed) b.pack_done();
        g_old_text = nullptr;
        const int rc = old::share_exchange_local(plans, 2);
        const char* why = a.refuses_exchange_local(a);
        if (!why) why = b.refuses_exchange_local(a);
        CHECK(same_text(rc ? g_old_text : nullptr, why));
      }
}

// ---- the widening: tables from the LCG, npolys in {15, 60}, strides up to 700, one row too long
void check_widen() {
  const int polys[] = {15, 60}, strides[] = {1, 7, 8, 9, 63, 64, 313, 700};
  for (int npolys : polys)
    for (int stride : strides)
      for (int too_long = 0; too_long < 2; ++too_long) {
        if (too_long && stride < 64) continue;
        std::snprintf(g_where, sizeof(g_where), "widen npolys=%d stride=%d too_long=%d", npolys, stride, too_long);
        Lcg lcg(7919ull * npolys + stride);
        std::vector<uint16_t> pos((size_t)npolys * stride);
        std::vector<int> npos((size_t)npolys);
        for (auto& q : pos) q = (uint16_t)(lcg.next() % 19937u);
        for (auto& n : npos) n = (int)(lcg.next() % (unsigned)(stride + 1));
        npos[0] = stride;                                   // a full row
        if (too_long) npos[1] = stride + 40;                // (reads on into row 2: inside the array)
        std::vector<uint32_t> wide;
        std::vector<int> counts;
        int wstride = 0;
        g_old_text = nullptr;
        const int rc = old::set_jump_widen(npolys, pos.data(), npos.data(), stride, wide, counts, wstride);
        const rfc::WideTable w = rfc::widen_jump_table(npolys, pos.data(), npos.data(), stride);
        CHECK(rc == too_long);
        CHECK(same_text(rc ? g_old_text : nullptr, w.refusal));
        if (rc) continue;
        CHECK(w.wstride == wstride && w.rows == wide && w.counts == counts);
      }
  // "a table has been uploaded": `p->mt_pos.get() && !p->mt_npos.empty()`
  rfc::JumpTable tab;
  int dev = 0;
  CHECK(!tab.uploaded(nullptr) && !tab.uploaded(&dev));
  tab.npos.assign(15, 1);
  CHECK(!tab.uploaded(nullptr) && tab.uploaded(&dev));
}

int print_geom(int nx, int ny, int nz, int bps) {
  const rfc::ReplayGeom g = rfc::replay_geom((unsigned long long)nx * ny * (nz / 2 + 1), bps, 16, true);
  std::printf("%d %d %lld %llu\n", g.nseg, g.stages, g.total_blocks - (long long)(g.nseg - 1) * bps, g.cap);
  return 0;
}
int print_split(int nseg, int nranks) {
  for (int r = 0; r < nranks; ++r) std::printf("%d%c", rfc::sh_seg_begin(r, nseg, nranks), r + 1 < nranks ? ' ' : '\n');
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 6 && !std::strcmp(argv[1], "geom")) return print_geom(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]));
  if (argc == 4 && !std::strcmp(argv[1], "split")) return print_split(std::atoi(argv[2]), std::atoi(argv[3]));
  if (argc != 1) { std::printf("usage: replay_test [geom nx ny nz bps | split nseg nranks]\n"); return 2; }
  struct { const char* name; long long checks; } done[8];
  int n = 0;
  auto section = [&](const char* name, long long before) { done[n].name = name; done[n].checks = g_checks - before; ++n; };
  long long c0 = g_checks;
  check_geom(); section("geometry", c0); c0 = g_checks;
  check_tree(16, 70000); check_tree(2, 4097); section("tree", c0); c0 = g_checks;
  check_hops(16, 70000, 4); check_hops(2, 4097, 13); section("hops", c0); c0 = g_checks;
  check_split(); section("split", c0); c0 = g_checks;
  check_step(); section("step", c0); c0 = g_checks;
  check_widen(); section("widening", c0);
  for (int i = 0; i < n; ++i) std::printf("%s: %lld checks\n", done[i].name, done[i].checks);
  std::printf("%lld checks, %lld failed\n", g_checks, g_failed);
  if (g_failed) return 1;
  std::printf("all checks passed\n");
  return 0;
}
