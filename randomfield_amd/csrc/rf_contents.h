// rf_contents.h -- what a plan's device buffers hold: the one record behind every refusal that keeps a call from reading garbage ("no
// real-space field on the device", "no k-space data", "no realisation has been computed", "no auxiliary field", "no second-order
// potential", "no painted counts", "no stashed spectrum", "no deviates resident").  The entry points ask it through the predicates and change it through the
// named transitions, one call per event; nothing else writes it.  Allocation ("is there a buffer at all": K.ptr, P.ptr, L.ptr, A.ptr ...)
// is not its business and stays with the buffers.  Plain C++, no HIP (tests/contents_test.cpp walks it on the CPU); the buffers are
// opaque addresses that are never dereferenced here.  DESIGN.md section 3.19 has the table in words.
#pragma once

namespace rfc {

struct Contents {
  // ---- predicates: one per meaning a refusal has -------------------------------------------------------------------------------
  bool field() const { return real_; }                                         // a real-space field, in whichever buffer (it always has one)
  bool field_in(const void* buf) const { return real_ && where_ == buf; }      // ... in this one (the in-place forward transforms: W)
  bool moments() const { return moments_; }                                    // the (sum, sumsq) pair moments_pair() of `stats` is the field's
  bool kspace() const { return k_ == K::spectrum; }                            // the K allocation holds a half spectrum
  bool aux() const { return k_ == K::aux; }                                    // ... an auxiliary REAL field (the lensing potential)
  bool potential2() const { return p2_; }                                      // L holds the second-order potential of the stored one
  bool counts() const { return counts_; }                                      // A holds the counts of a paint
  bool stash() const { return stash_; }                                        // the stash holds a half spectrum put aside by rf_kspace_stash
  bool deviates64() const { return dev_ == Dev::f64; }                         // `noise` holds float64 deviates in cell order
  bool deviates32() const { return dev_ == Dev::f32; }                         // the replay's runs hold float32 pairs
  bool deviates() const { return dev_ != Dev::none; }
  // the buffer of the last field (kept when the field goes; null before the first) and the pair its moments are read from
  void* where() const { return where_; }
  int moments_pair() const { return slot_; }

  // ---- transitions ------------------------------------------------------------------------------------------------------------
  // the field                               buffer        a field there     its moments        their pair
  void field_ready(void* buf, int pair)    { where_ = buf; real_ = true;     moments_ = true;   slot_ = pair; }     // a realisation, a c2r
  void field_written(void* buf)            { where_ = buf; real_ = true;     moments_ = false; }                    // upload, paint, 2LPT source
  void field_gathered(void* buf)           { where_ = buf; real_ = true; }                                          // the gathering z pass: the moments are its caller's
  void field_modified()                    {                                 moments_ = false; }                    // changed in place
  void field_consumed()                    {               real_ = false;    moments_ = false; }                    // an in-place forward transform took it
  void not_a_field()                       {               real_ = false; }                                         // stand-in exchange, new chunking, rows cut for the reverse exchange
  void moments_ready(int pair)             {                                 moments_ = true;   slot_ = pair; }
  void moments_moved(int pair)             {                                                    slot_ = pair; }     // rf_slab_backward: the pair alone, claimed or not as before
  // the K allocation: a half spectrum, an auxiliary real field, or neither
  void kspace_ready()                      { k_ = K::spectrum; }
  void kspace_consumed()                   { if (k_ == K::spectrum) k_ = K::nothing; }      // (an auxiliary field stays one)
  void aux_ready()                         { k_ = K::aux; }
  void kside_cleared()                     { k_ = K::nothing; }                             // rf_lpt2_source, whichever kind of plan
  // the deviates: float64 in cell order, float32 pairs in the runs, or neither
  void deviates_none()                     { dev_ = Dev::none; }
  void deviates64_ready()                  { dev_ = Dev::f64; }
  void deviates32_ready()                  { dev_ = Dev::f32; }
  void deviates64_dropped()                { if (dev_ == Dev::f64) dev_ = Dev::none; }      // the noise buffer is about to grow
  // the second-order potential and the painted counts
  void potential2_ready()                  { p2_ = true; }
  void potential2_stale()                  { p2_ = false; }
  void counts_ready()                      { counts_ = true; }
  void counts_stale()                      { counts_ = false; }
  // the stashed half spectrum: the caller's data, so nothing but the plan's end makes it stale -- there is no way back
  void stash_ready()                       { stash_ = true; }

 private:
  enum class K { nothing, spectrum, aux };
  enum class Dev { none, f64, f32 };
  void* where_ = nullptr;
  int slot_ = 0;
  bool real_ = false, moments_ = false, p2_ = false, counts_ = false, stash_ = false;
  K k_ = K::nothing;
  Dev dev_ = Dev::none;
};

}  // namespace rfc
