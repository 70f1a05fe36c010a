// uis_blob.h -- the blob of uis_stream_export / uis_stream_import (uis_migrate.hip): one utterance of a streaming
// session between two pushes, as bytes.  Plain C++: the header, the section arithmetic, the hash and the host's
// validator, no HIP type -- tests/blob_check_main.cpp builds it with the host compiler alone.
//
// Layout (little endian, every section starts 16-byte aligned, every pad byte is zero):
//   header    UisBlobHeader, 64 bytes: magic, format version, UIS_NUMERICS_VERSION, look_ahead (1), the session's shape
//             B, D, Dp, H, Hp, depth, the HidMap segment pair, the 64-bit hash of the model's parameters, total bytes
//   scalars   UisBlobScalars, 32 bytes: committed, N (window frames = utt_step), live, n (distinct pool slots),
//             lists (= sum of K over the live ranks), win_score
//   ranks     [live] x {K, last, sum, score bits}: 16 bytes per live rank, best first.  `last` is the last-label word:
//             the label in bits 0 .. 15 (signed; -1 exactly where K = 0), and in bits 16 .. 30 the hypothesis' run under
//             its slot's minimum turn length (uis_session_min_turn): 0 in a stream from a slot without a rule, whose
//             blob is unchanged.  The slot's value itself is not in the blob: import normalises the word against the
//             target slot's (uis_blob_last_word)
//   lists     rank by rank: K slot indices (renumbered into 0 .. n - 1), then K block-count words (the count, and in
//             bits 24 .. 30 the cluster's speaker tag: 0 in a stream without known speakers, whose blob is unchanged); int32
//   cnt       [n] int32: frames each slot's cluster has absorbed
//   mean      [n][Dp] float32: the pool's padded rows, as they are
//   hid       [n][depth][Hp] float32: the pool's padded / HidMap rows, as they are
//   records   [N][B] uint32: the record words of window steps [0, N), verbatim
//   trailer   16 bytes: uis_blob_hash of everything before it, then UIS_BLOB_END
// The blob is canonical: it is a function of the utterance's state alone (slots are numbered by ascending index in
// the source pool, which import reproduces, so export(import(b)) == b).
#ifndef UIS_BLOB_H_
#define UIS_BLOB_H_

#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define UIS_BLOB_FN __host__ __device__ inline
#else
#define UIS_BLOB_FN inline
#endif

#define UIS_BLOB_MAGIC 0x42534955u          // "UISB"
#define UIS_BLOB_FORMAT 1u
#define UIS_BLOB_END 0x444e454253495555ull  // "UUISBEND"
#define UIS_BLOB_MAX_BEAM 256               // (uis_stream_begin's limits)
#define UIS_BLOB_MAX_CLUSTERS 4096
#define UIS_BLOB_MAX_FRAMES 0x7fffff00ll
// a block-count word of the lists: the count in bits 0 .. 23, the cluster's speaker tag in bits 24 .. 30 (0: none) --
// uis_kernels.h's UIS_BLK_*, restated because this header stands alone
#define UIS_BLOB_BLK_TAG_SHIFT 24
#define UIS_BLOB_BLK_COUNT_MASK 0x00ffffff
// a last-label word of the ranks: uis_kernels.h's UIS_LAST_*, restated likewise
#define UIS_BLOB_LAST_RUN_SHIFT 16
#define UIS_BLOB_LAST_RUN_MASK 0x7fff

UIS_BLOB_FN int32_t uis_blob_last_label(int32_t w) { return (int32_t)(int16_t)(w & 0xffff); }
UIS_BLOB_FN int32_t uis_blob_last_run(int32_t w) { return (w >> UIS_BLOB_LAST_RUN_SHIFT) & UIS_BLOB_LAST_RUN_MASK; }

// A blob's last-label word as a slot whose minimum turn length is m holds it (uis_stream_import): no label stays -1; a
// slot without a rule (m < 2) holds the bare label; a word without a run comes from a slot without a rule -- nothing is
// known of the turn, so the past sets no constraint: run m --; else the run, saturated at m.
UIS_BLOB_FN int32_t uis_blob_last_word(int32_t w, int32_t m) {
  const int32_t label = uis_blob_last_label(w);
  if (w < 0 || label < 0) return -1;
  if (m < 2) return label;
  const int32_t run = uis_blob_last_run(w);
  return label | ((run == 0 || run > m ? m : run) << UIS_BLOB_LAST_RUN_SHIFT);
}

struct UisBlobHeader {
  uint32_t magic, format, numerics, look_ahead;
  int32_t B, D, Dp, H;
  int32_t Hp, depth, hid_seg, hid_seg_p;
  uint64_t model_hash;
  int64_t total_bytes;
};

struct UisBlobScalars {
  int64_t committed;
  int32_t N, live, n, lists;
  float win_score;
  int32_t zero;
};

struct UisBlobRank {
  int32_t K, last, sum;
  float score;
};

// what a session expects of a blob it is handed (the model fingerprint, the numerics, the beam)
struct UisBlobShape {
  uint32_t numerics;
  int32_t B, D, Dp, H, Hp, depth, hid_seg, hid_seg_p;
  uint64_t model_hash;
};

// byte offsets of the sections
struct UisBlobLayout {
  int64_t scalars, ranks, lists, cnt, mean, hid, records, trailer, total;
};

UIS_BLOB_FN int64_t uis_blob_align(int64_t x) { return (x + 15) & ~(int64_t)15; }

UIS_BLOB_FN UisBlobLayout uis_blob_layout(int64_t B, int64_t Dp, int64_t Hp, int64_t depth, int64_t N, int64_t live, int64_t n,
                                          int64_t lists) {
  UisBlobLayout l;
  l.scalars = (int64_t)sizeof(UisBlobHeader);
  l.ranks = l.scalars + (int64_t)sizeof(UisBlobScalars);
  l.lists = l.ranks + live * (int64_t)sizeof(UisBlobRank);
  l.cnt = uis_blob_align(l.lists + 2 * lists * 4);
  l.mean = uis_blob_align(l.cnt + n * 4);
  l.hid = l.mean + n * Dp * 4;
  l.records = l.hid + n * depth * Hp * 4;
  l.trailer = uis_blob_align(l.records + N * B * 4);
  l.total = l.trailer + 16;
  return l;
}

// The most a blob of a session of this shape can take: every rank live with max_clusters clusters, every one of the
// S pool slots named, a full window.
inline int64_t uis_blob_bound(int64_t B, int64_t Dp, int64_t Hp, int64_t depth, int64_t max_frames, int64_t max_clusters, int64_t S) {
  return uis_blob_layout(B, Dp, Hp, depth, max_frames, B, S, B * max_clusters).total;
}

// 64-bit hash over 8-byte words in four lanes, every step a bijection of the lane (a change of one word always
// changes the result); a tail of fewer than 8 bytes is zero-extended.  Host only.
inline uint64_t uis_blob_hash(const void* data, size_t bytes, uint64_t seed) {
  const unsigned char* p = static_cast<const unsigned char*>(data);
  const uint64_t prime = 0x100000001b3ull;
  uint64_t lane[4] = {seed ^ 0xcbf29ce484222325ull, seed ^ 0x9e3779b97f4a7c15ull, seed ^ 0xc2b2ae3d27d4eb4full, seed ^ 0x165667b19e3779f9ull};
  const size_t words = bytes / 8;
  size_t i = 0;
  for (; i + 4 <= words; i += 4) {
    uint64_t w[4];
    memcpy(w, p + i * 8, 32);
    for (int k = 0; k < 4; ++k) lane[k] = (lane[k] ^ w[k]) * prime;
  }
  for (int k = 0; i < words; ++i, ++k) {
    uint64_t w;
    memcpy(&w, p + i * 8, 8);
    lane[k] = (lane[k] ^ w) * prime;
  }
  if (bytes & 7) {
    uint64_t w = 0;
    memcpy(&w, p + words * 8, bytes & 7);
    lane[3] = (lane[3] ^ w) * prime;
  }
  uint64_t hsh = (uint64_t)bytes;
  for (int k = 0; k < 4; ++k) hsh = ((hsh ^ lane[k]) * prime) ^ (hsh >> 29);
  return hsh;
}

// Close a blob whose sections are written: the total in the header, the hash and the end word in the trailer.
inline void uis_blob_seal(void* blob, const UisBlobLayout& l) {
  char* b = static_cast<char*>(blob);
  UisBlobHeader hd;
  memcpy(&hd, b, sizeof(hd));
  hd.total_bytes = l.total;
  memcpy(b, &hd, sizeof(hd));
  const uint64_t tr[2] = {uis_blob_hash(b, (size_t)l.trailer, 0), UIS_BLOB_END};
  memcpy(b + l.trailer, tr, 16);
}

struct UisBlobInfo {
  UisBlobHeader hd;
  UisBlobScalars sc;
  UisBlobLayout lay;
  int32_t max_K;
  int32_t max_tag;   // the largest speaker tag a live rank has bound (0: the blob carries none)
  int32_t max_run;   // the largest run a live rank's last-label word carries (0: the blob comes from a slot without a minimum turn length)
};

enum {
  UIS_BLOB_OK = 0,
  UIS_BLOB_MALFORMED = 1,  // not a blob, cut short, damaged, or inconsistent in itself
  UIS_BLOB_MISMATCH = 2    // a well-formed blob of another model, numerics version or beam
};

// Everything that could steer a device address or a loop bound of the import kernels, checked on the host; record
// words are not looked at (their readers clamp).  `expect` null: the blob's own consistency only.  `why`: a constant
// string naming the first complaint.
inline int uis_blob_validate(const void* blob, int64_t bytes, const UisBlobShape* expect, UisBlobInfo* info, const char** why) {
  const char* dummy;
  if (!why) why = &dummy;
  *why = "";
  if (!blob || bytes < (int64_t)(sizeof(UisBlobHeader) + sizeof(UisBlobScalars) + 16)) { *why = "shorter than an empty blob"; return UIS_BLOB_MALFORMED; }
  const char* b = static_cast<const char*>(blob);
  UisBlobInfo in;
  memcpy(&in.hd, b, sizeof(in.hd));
  memcpy(&in.sc, b + sizeof(in.hd), sizeof(in.sc));
  const UisBlobHeader& hd = in.hd;
  const UisBlobScalars& sc = in.sc;
  if (hd.magic != UIS_BLOB_MAGIC) { *why = "bad magic"; return UIS_BLOB_MALFORMED; }
  if (hd.format != UIS_BLOB_FORMAT) { *why = "unknown blob format version"; return UIS_BLOB_MALFORMED; }
  if (hd.total_bytes != bytes) { *why = "the header's size is not the size given (truncated?)"; return UIS_BLOB_MALFORMED; }
  if (hd.look_ahead != 1u) { *why = "look_ahead is not 1"; return UIS_BLOB_MALFORMED; }
  if (hd.B < 1 || hd.B > UIS_BLOB_MAX_BEAM || hd.D < 1 || hd.H < 1 || hd.depth < 1 || hd.depth > 8 || hd.Dp < hd.D || hd.Hp < hd.H ||
      (hd.Dp & 15) || (hd.Hp & 15) || hd.Dp > (1 << 20) || hd.Hp > (1 << 20) || hd.hid_seg < 0 || hd.hid_seg_p < 0)
    { *why = "impossible shape in the header"; return UIS_BLOB_MALFORMED; }
  if (sc.zero != 0) { *why = "reserved word is not zero"; return UIS_BLOB_MALFORMED; }
  if (sc.N < 0 || (int64_t)sc.N > UIS_BLOB_MAX_FRAMES || sc.committed < 0 || sc.committed + sc.N > UIS_BLOB_MAX_FRAMES)
    { *why = "frame counts out of range"; return UIS_BLOB_MALFORMED; }
  if (sc.live < 1 || sc.live > hd.B) { *why = "live hypotheses not in [1, beam_size]"; return UIS_BLOB_MALFORMED; }
  if (sc.lists < 0 || (int64_t)sc.lists > (int64_t)sc.live * UIS_BLOB_MAX_CLUSTERS || sc.n < 0 || sc.n > sc.lists)
    { *why = "slot or list counts out of range"; return UIS_BLOB_MALFORMED; }
  in.lay = uis_blob_layout(hd.B, hd.Dp, hd.Hp, hd.depth, sc.N, sc.live, sc.n, sc.lists);
  const UisBlobLayout& l = in.lay;
  if (l.total != bytes) { *why = "section sizes do not add up to the size given"; return UIS_BLOB_MALFORMED; }
  uint64_t tr[2];
  memcpy(tr, b + l.trailer, 16);
  if (tr[1] != UIS_BLOB_END) { *why = "bad end word"; return UIS_BLOB_MALFORMED; }
  if (tr[0] != uis_blob_hash(b, (size_t)l.trailer, 0)) { *why = "checksum mismatch"; return UIS_BLOB_MALFORMED; }
  // ---- the ranks and their lists
  int64_t at = 0;
  in.max_K = 0;
  in.max_tag = 0;
  in.max_run = 0;
  int runless = 0;   // ranks that have a label and no run
  for (int r = 0; r < sc.live; ++r) {
    UisBlobRank rk;
    memcpy(&rk, b + l.ranks + (int64_t)r * (int64_t)sizeof(rk), sizeof(rk));
    if (rk.K < 0 || rk.K > UIS_BLOB_MAX_CLUSTERS || at + rk.K > sc.lists) { *why = "a rank's cluster count is out of range"; return UIS_BLOB_MALFORMED; }
    // (the label of the word; a word without a label is -1 exactly, and a hypothesis that has clusters has a label)
    if (rk.K == 0 ? rk.last != -1 : (rk.last < 0 || uis_blob_last_label(rk.last) < 0 || uis_blob_last_label(rk.last) >= rk.K))
      { *why = "a rank's last label is not one of its clusters"; return UIS_BLOB_MALFORMED; }
    // (all live ranks come from one slot: under its minimum turn length every rank that has a label has a run of 1 or
    // more, without one none has run bits.  The run itself is not bounded by the stream: a word that arrived without a
    // run holds the slot's value, however short the stream.  So the run of a LONE rank is unchecked by design: import
    // clamps it against the target slot's value)
    if (rk.K > 0) {
      const int32_t run = uis_blob_last_run(rk.last);
      if (run > 0 ? runless > 0 : in.max_run > 0) { *why = "the ranks disagree on whether their slot has a minimum turn length"; return UIS_BLOB_MALFORMED; }
      runless += run == 0;
      if (run > in.max_run) in.max_run = run;
    }
    int64_t sum = 0;
    uint64_t seen[2] = {0, 0};   // the tags this rank has bound
    for (int k = 0; k < rk.K; ++k) {
      int32_t slot, blk;
      memcpy(&slot, b + l.lists + (2 * at + k) * 4, 4);
      memcpy(&blk, b + l.lists + (2 * at + rk.K + k) * 4, 4);
      if (slot < 0 || slot >= sc.n) { *why = "a slot index is not below the slot count"; return UIS_BLOB_MALFORMED; }
      if (blk < 0) { *why = "a negative block count"; return UIS_BLOB_MALFORMED; }
      sum += blk & UIS_BLOB_BLK_COUNT_MASK;
      const int tag = blk >> UIS_BLOB_BLK_TAG_SHIFT;   // (0 .. 127: blk is not negative)
      if (!tag) continue;
      if ((seen[tag >> 6] >> (tag & 63)) & 1u) { *why = "a tag bound twice"; return UIS_BLOB_MALFORMED; }
      seen[tag >> 6] |= (uint64_t)1 << (tag & 63);
      if (sc.committed + sc.N >= ((int64_t)1 << UIS_BLOB_BLK_TAG_SHIFT))
        { *why = "a tag in a stream of 2^24 frames or more (it shares the block-count word)"; return UIS_BLOB_MALFORMED; }
      if (tag > in.max_tag) in.max_tag = tag;
    }
    if (sum != (int64_t)rk.sum || sum > sc.committed + sc.N) { *why = "a rank's block counts do not add up to its sum"; return UIS_BLOB_MALFORMED; }
    at += rk.K;
    if (rk.K > in.max_K) in.max_K = rk.K;
  }
  if (at != sc.lists) { *why = "the ranks' cluster counts do not add up to the list length"; return UIS_BLOB_MALFORMED; }
  for (int j = 0; j < sc.n; ++j) {
    int32_t c;
    memcpy(&c, b + l.cnt + (int64_t)j * 4, 4);
    if (c < 1 || (int64_t)c > sc.committed + sc.N) { *why = "a slot's frame count is not in [1, frames received]"; return UIS_BLOB_MALFORMED; }
  }
  // ---- the pads
  auto zeros = [&](int64_t from, int64_t to) {
    for (int64_t i = from; i < to; ++i)
      if (b[i]) return false;
    return true;
  };
  if (!zeros(l.lists + 2 * (int64_t)sc.lists * 4, l.cnt) || !zeros(l.cnt + (int64_t)sc.n * 4, l.mean) ||
      !zeros(l.records + (int64_t)sc.N * hd.B * 4, l.trailer))
    { *why = "a pad byte is not zero"; return UIS_BLOB_MALFORMED; }
  if (info) *info = in;
  if (expect) {
    if (hd.numerics != expect->numerics) { *why = "the blob was written under another UIS_NUMERICS_VERSION"; return UIS_BLOB_MISMATCH; }
    if (hd.B != expect->B) { *why = "the blob's beam_size is not the session's"; return UIS_BLOB_MISMATCH; }
    if (hd.D != expect->D || hd.Dp != expect->Dp || hd.H != expect->H || hd.Hp != expect->Hp || hd.depth != expect->depth ||
        hd.hid_seg != expect->hid_seg || hd.hid_seg_p != expect->hid_seg_p || hd.model_hash != expect->model_hash)
      { *why = "the blob belongs to another model (fingerprint mismatch)"; return UIS_BLOB_MISMATCH; }
  }
  return UIS_BLOB_OK;
}

#endif  // UIS_BLOB_H_
