// rf_replay.h -- the host side of the on-GPU replay of np.random.RandomState(seed).normal: what the uploaded jump table is, the sizes of
// one replay, the order in which the jump tree is grown, the hops to a rank's first segment, which cells of the one stream every rank of
// a kz-slab job sends to every other, and the step the shared replay is at.  The entry points of rf_capi_mt.hip call these and keep the
// HIP calls; the kernels are rf_k_mt.hip.  Plain C++, no HIP (tests/replay_test.cpp holds every function against the expressions it
// replaced, on the CPU).  A function that can refuse hands the refusal's text back (nullptr: none); the entry point fails with it.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rfc {

// ---- the jump table -----------------------------------------------------------------------------------------------------------------
struct ReplayGeom;
// what rf_mt_set_jump keeps on the host: row t (R - 1) + m - 1 is the polynomial t^(m R^t L) of a segment of L = bps blocks of 624 words
struct JumpTable {
  std::vector<int> npos;          // set bits per polynomial, as uploaded (its length: the polynomials the table has)
  int stride = 0;                 // entries per device row (widen_jump_table's wstride)
  int bps = 0, radix = 2;         // blocks per segment, tree radix R
  // `device_rows`: the device copy of the rows (null until an upload has succeeded; never dereferenced here)
  bool uploaded(const void* device_rows) const { return device_rows && !npos.empty(); }
  inline const char* refuses(const ReplayGeom& g) const;
};

// The device rows (rf_k_mt.hip mt_jump_kernel): four lists, one per class c = position mod 4, each padded to a multiple of 8 entries; an
// entry is the byte offset 4 (position - c) of an aligned 16-byte read; the padding points into the block of zero words behind the
// 33-block window (33 * 624 words); four padded counts per polynomial.
struct WideTable {
  std::vector<uint32_t> rows;     // [npolys][wstride]
  std::vector<int> counts;        // [npolys][4]
  int wstride = 0;
  const char* refusal = nullptr;
};
inline WideTable widen_jump_table(int npolys, const uint16_t* pos, const int* npos, int stride) {
  WideTable w;
  const uint32_t null_off = 4u * 33u * 624u;
  w.wstride = ((stride + 7) / 8 + 4) * 8;
  w.rows.assign((size_t)npolys * w.wstride, null_off);
  w.counts.resize(4 * (size_t)npolys);
  for (int l = 0; l < npolys; ++l) {
    int n[4] = {0, 0, 0, 0};
    for (int j = 0; j < npos[l]; ++j) ++n[pos[(size_t)l * stride + j] & 3];
    int off[4], padded[4];
    for (int c = 0, o = 0; c < 4; ++c) { padded[c] = (n[c] + 7) & ~7; off[c] = o; o += padded[c]; }
    if (off[3] + padded[3] > w.wstride) { w.refusal = "jump table row too long"; return w; }
    int k[4] = {0, 0, 0, 0};
    for (int j = 0; j < npos[l]; ++j) {
      const uint32_t q = pos[(size_t)l * stride + j];
      const int c = (int)(q & 3u);
      w.rows[(size_t)l * w.wstride + off[c] + k[c]++] = 4u * (q - (uint32_t)c);
    }
    for (int c = 0; c < 4; ++c) w.counts[4 * l + c] = padded[c];
  }
  return w;
}

// ---- geometry -----------------------------------------------------------------------------------------------------------------------
// stages of the radix-R jump tree over nseg segments: stage t turns the start states of segments [0, R^t) into those of [R^t, R^(t+1))
inline int tree_stages(int nseg, int radix) {
  int stages = 0;
  for (long long reach = 1; reach < nseg; reach *= radix) ++stages;
  return stages;
}

// sizes of one replay of RandomState(seed).normal for a grid of ncells = nx ny (nz/2 + 1) cells
struct ReplayGeom {
  unsigned long long ncells = 0, attempts = 0, cap = 0;     // cap: attempts (= slots of its run) per segment
  long long total_blocks = 0;
  int nseg = 0, stages = 0;
  size_t need = 0;                // bytes of the runs: nseg * cap pairs
};
inline ReplayGeom replay_geom(unsigned long long ncells, int bps, int radix, bool single) {
  ReplayGeom g;
  g.ncells = ncells;
  // polar attempts to generate: acceptance pi/4, margin of 10 sigma + 1024 (mt19937.attempts_needed)
  const double pa = 0.78539816339744830962;
  g.attempts = (unsigned long long)std::ceil((double)ncells / pa + 10.0 * std::sqrt((double)ncells * (1 - pa)) / pa + 1024.0);
  g.total_blocks = (long long)((4 * g.attempts + 623) / 624);
  g.nseg = (int)((g.total_blocks + bps - 1) / bps);
  g.stages = tree_stages(g.nseg, radix);
  g.cap = (unsigned long long)bps * (624 / 4);
  g.need = (size_t)g.nseg * g.cap * (single ? 2 * sizeof(float) : 2 * sizeof(double));
  return g;
}
// stage t needs the R - 1 polynomials t^(m R^t L), rows t (R - 1) .. of the table
inline const char* JumpTable::refuses(const ReplayGeom& g) const {
  return g.stages * (radix - 1) <= (int)npos.size() ? nullptr : "grid too large for the uploaded jump table";
}
// the float32 form locates a row's pairs through a table that allows ONE segment boundary per row: segments (cap attempts,
// ~0.785 cap pairs) must be longer than a row (nzh = nz/2 + 1 cells) by a wide margin, or the float64 form (moved into cell order) serves
inline bool pairs32_fit(const ReplayGeom& g, int nzh) { return g.cap >= 4ull * (unsigned long long)nzh; }

// ---- the jump tree ------------------------------------------------------------------------------------------------------------------
// Stage t jumps the nsrc = R^t states of segments [0, dist) by m dist segments, m = 1 .. R - 1 (rows t (R - 1) .. of the table);
// destinations at or behind nseg are the kernel's to drop.  f(t, nsrc, dist) is called once per stage, in order, and returns 0 to go on;
// anything else ends the walk and is handed back.  The whole stream calls it with its nseg, a rank of the shared replay with the number
// of its own segments.
template <class F>
inline int for_each_tree_stage(int nseg, int radix, F&& f) {
  long long dist = 1;
  for (int t = 0; dist < nseg; ++t, dist *= radix)
    if (int rc = f(t, (int)dist, dist)) return rc;      // (dist < nseg: every source exists)
  return 0;
}

// ---- the hops to a rank's first segment ---------------------------------------------------------------------------------------------
// The start state of segment `first`: one jump per non-zero radix-R digit of `first` (digit d of weight R^t: row t (R - 1) + d - 1 of the
// table), hopping through the spare state slots behind the rank's own -- hop i reads spare slot i and writes spare slot i + 1.
constexpr int kSpareSlots = 8;
struct Hops {
  int rows[kSpareSlots - 1];
  int n = 0;
  const char* refusal = nullptr;
};
inline Hops digit_hops(int first, int radix, int stages) {
  Hops h;
  int rest = first;
  for (int t = 0; rest > 0; ++t, rest /= radix) {
    const int d = rest % radix;
    if (d == 0) continue;
    if (!(t < stages && h.n + 1 < kSpareSlots)) { h.refusal = "segment index beyond the uploaded jump table"; return h; }
    h.rows[h.n++] = t * (radix - 1) + d - 1;
  }
  return h;
}

// ---- the split of the one stream between the ranks of a kz-slab job -----------------------------------------------------------------
// rank r replays segments [sh_seg_begin(r), sh_seg_begin(r + 1))
inline int sh_seg_begin(int r, int nseg, int nranks) { return (int)((long long)r * nseg / nranks); }

// the index in "stream q" (rows of nzl + 1 pairs: q's planes, then the Nyquist plane) of the first stream-q cell at or behind stream cell c
inline unsigned long long stream_index(int q, unsigned long long c, int nzl, int nzh) {
  const unsigned long long col = c / (unsigned)nzh;
  long long k = (long long)(c - col * (unsigned)nzh) - (long long)q * nzl;
  k = k < 0 ? 0 : (k > nzl ? nzl : k);
  return col * (unsigned)(nzl + 1) + (unsigned long long)k;
}

// everything rf_mt_share_pack works out on the host from the gathered counts; offsets and counts are in pairs, per peer
struct ShareSplit {
  std::vector<unsigned long long> first;      // [nseg + 1]: first stream cell of every segment; first[nseg] == total
  unsigned long long total = 0;               // accepted pairs of the whole stream
  std::vector<unsigned long long> sendoff, sendcnt, recvoff, recvcnt;      // sendoff: [nranks + 1], the others [nranks]
  std::vector<long long> sbase;               // [nranks]: see mt_share_pack_kernel
  const char* refusal = nullptr;
};
inline ShareSplit share_split(const unsigned long long* counts_all, const ReplayGeom& g, int nranks, int rank, int nzl, int nzh) {
  ShareSplit s;
  const int P = nranks, me = rank;
  s.first.resize((size_t)g.nseg + 1);
  s.first[0] = 0;
  for (int i = 0; i < g.nseg; ++i) {
    if (counts_all[i] > g.cap) { s.refusal = "a segment cannot hold more pairs than attempts: the gathered counts are corrupt"; return s; }
    s.first[i + 1] = s.first[i] + counts_all[i];
  }
  if (s.first[g.nseg] < g.ncells) { s.refusal = "MT19937 replay: not enough accepted polar attempts (increase the margin)"; return s; }
  s.total = s.first[g.nseg];
  // first cell of every rank's share
  std::vector<unsigned long long> cb((size_t)P + 1);
  for (int r = 0; r <= P; ++r) {
    const unsigned long long c = s.first[sh_seg_begin(r, g.nseg, P)];
    cb[r] = c < g.ncells ? c : g.ncells;
  }
  cb[P] = g.ncells;
  auto fq = [&](int q, unsigned long long c) { return stream_index(q, c, nzl, nzh); };
  s.sendoff.assign(P + 1, 0); s.sendcnt.assign(P, 0); s.recvoff.assign(P, 0); s.recvcnt.assign(P, 0);
  s.sbase.assign(P, 0);
  for (int q = 0; q < P; ++q) {
    s.sendcnt[q] = fq(q, cb[me + 1]) - fq(q, cb[me]);
    s.sendoff[q + 1] = s.sendoff[q] + s.sendcnt[q];
    s.sbase[q] = (long long)s.sendoff[q] - (long long)fq(q, cb[me]);
    s.recvoff[q] = fq(me, cb[q]);                       // (q = the sending rank here)
    s.recvcnt[q] = fq(me, cb[q + 1]) - fq(me, cb[q]);
  }
  return s;
}

// ---- the step of the shared replay --------------------------------------------------------------------------------------------------
// rf_mt_share_begin -> (gather) -> pack -> exchange / exchange_local -> finish.  The entry points ask through the refusals and change it
// through the named transitions; nothing else writes it.  The precision of the transport (float32 pairs or float64 deviates) is
// fixed by the replay and goes with the step.
struct ShareStep {
  bool idle() const { return s_ == S::idle; }
  bool replayed() const { return s_ == S::replayed; }
  bool packed() const { return s_ == S::packed; }
  bool exchanged() const { return s_ == S::exchanged; }
  bool single() const { return single_; }                   // of the last replay (kept when the step goes back to idle)

  // the text a call is refused with at this step (nullptr: it may go on)
  const char* refuses_gather() const { return replayed() ? nullptr : "rf_mt_share_begin must be called first"; }
  const char* refuses_pack() const { return refuses_gather(); }
  const char* refuses_exchange() const { return packed() ? nullptr : "rf_mt_share_pack must be called first"; }
  // ... between virtual ranks: every plan packed, in the mode of rank 0
  const char* refuses_exchange_local(const ShareStep& rank0) const {
    return packed() && single_ == rank0.single_ ? nullptr : "rf_mt_share_pack must have run on every plan (same mode)";
  }
  const char* refuses_finish() const { return exchanged() ? nullptr : "the exchange must have run first"; }

  void reset()                     { s_ = S::idle; }                             // rf_mt_share_begin, before it can fail
  void replay_done(bool single)    { s_ = S::replayed; single_ = single; }
  void pack_done()                 { s_ = S::packed; }
  void exchange_done()             { s_ = S::exchanged; }
  void finish_done()               { s_ = S::idle; }

 private:
  enum class S { idle, replayed, packed, exchanged };
  S s_ = S::idle;
  bool single_ = false;
};

}  // namespace rfc
