// uis_push_layout.h -- where things lie in the two blocks a streaming push fills, and the rows of the chunk each
// utterance reads (uis_stream.hip).  Plain C++: byte arithmetic and typed views over a base
// pointer, no HIP type -- tests/push_layout_main.cpp builds it with the host compiler alone.
//
//   MailboxLayout   the host-coherent block of a UIS_FLAG_PERSISTENT session: the control words, then eight regions,
//                   each 128-byte aligned, in this order: foff, avail, lab_off, scores, beam_scores, overflow, frames,
//                   labels; every cluster's fixed row range of the frame area (and of the chunk buffers)
//   ChunkLayout     the staging block of a push through ordinary launches, mirrored at the front of the chunk's x
//                   buffer: [k_ingest's table, tensors only][foff U x int64][avail U x int32, padded to 16][frames]
//   chunk_rows*     foff / avail of a push from its counts and the window's `have`: the only place they are formed
#ifndef UIS_PUSH_LAYOUT_H_
#define UIS_PUSH_LAYOUT_H_

#include <stddef.h>
#include <stdint.h>

// The one typed view: T at byte `o` of the block at `base` (the host's pointer or the device's), e.g.
// uis_block_at<int64_t>(pm, box.o_foff).  foff, lab_off: int64; avail, overflow, labels: int32; scores, beam_scores,
// frames: float.
template <typename T>
inline T* uis_block_at(void* base, size_t o) { return reinterpret_cast<T*>(static_cast<unsigned char*>(base) + o); }

struct MailboxLayout {
  size_t o_foff = 0, o_avail = 0, o_lab_off = 0, o_scores = 0, o_beam_scores = 0, o_overflow = 0, o_frames = 0, o_labels = 0, total = 0;
  // cluster_rows: every cluster gets a FIXED row range of the chunk buffers (x, gi0, mse0) and of the frame area: room
  // for 16 frames of each of its utterances, whole pairs of 16-row tiles, at most rows_max (uis_stream_begin says why it
  // must be fixed); cap_frames: rows of the frame area = ncl * cluster_rows; hdr_stride: of the device's per-cluster
  // copies of [foff U x 8][avail U x 4] (PersistArgs::hdr)
  int64_t cluster_rows = 0, cap_frames = 0;
  size_t hdr_stride = 0;

  MailboxLayout() = default;
  // ctl_words: the control words in front (UIS_PM_CTL_WORDS); rows_max: the one-launch kernel's row list
  MailboxLayout(int U, int B, int D, int64_t max_frames, int ncl, size_t ctl_words, int64_t rows_max) {
    cluster_rows = ((int64_t)((U + ncl - 1) / ncl) * 16 + 31) / 32 * 32;
    if (cluster_rows > rows_max) cluster_rows = rows_max;
    cap_frames = cluster_rows * ncl;
    size_t o = ctl_words * 4;
    const auto take = [&o](size_t bytes) { o = (o + 127) & ~(size_t)127; const size_t r = o; o += bytes; return r; };
    o_foff = take((size_t)U * 8);
    o_avail = take((size_t)U * 4);
    o_lab_off = take((size_t)U * 8);
    o_scores = take((size_t)U * 4);
    o_beam_scores = take((size_t)U * B * 4);
    o_overflow = take((size_t)U * 4);
    o_frames = take((size_t)cap_frames * D * 4);
    o_labels = take((size_t)U * (size_t)max_frames * 4);
    total = o;
    hdr_stride = (((size_t)U * 12) + 127) & ~(size_t)127;
  }
};

struct ChunkLayout {
  // F frames, one chunk row each.  o_foff: also the size of k_ingest's table in front (0 for host
  // frames; a multiple of 16: the rest lies as it did); travel_bytes: what the one H2D carries -- header and frames, or
  // the header alone (the gather writes the frames); total_bytes: what the chunk's x buffer must hold
  size_t o_foff = 0, o_avail = 0, o_frames = 0, travel_bytes = 0, total_bytes = 0;

  // table_stride: the bytes of one row of k_ingest's table
  ChunkLayout(int U, int64_t F, int D, bool tensors, size_t table_stride) {
    o_foff = tensors ? (size_t)U * table_stride : 0;
    o_avail = o_foff + (size_t)U * 8;
    // (avail alone is padded, so the frame area is 16-byte aligned for an even U only: for an odd one U * 8 leaves it on
    // an 8-byte boundary, where k_ingest takes its element-by-element path.  Kept as it was: DESIGN.md section 32)
    o_frames = o_avail + (((size_t)U * 4 + 15) & ~(size_t)15);
    total_bytes = o_frames + (size_t)F * D * 4;
    travel_bytes = tensors ? o_frames : total_bytes;
  }
};

// ---- the chunk's rows.  Utterance u's new frames are counts[u] consecutive rows; step s of the utterance (counted
// from the window's start, of which have[u] steps are run) reads row foff[u] + s, and the utterance has avail[u] frames.
// Cluster by cluster (cluster c owns utterances c, c + ncl, ...), each from the start of its fixed range of
// cluster_rows rows: a push through the mailbox, whose clusters fetch ONE contiguous row range each -- rows
// [row0[c], row0[c] + nrow[c]).  A push through ordinary launches is the case of one cluster from row 0 (ncl 1,
// cluster_rows 0), utterance after utterance.  Returns whether every cluster's share fits its range.  Null outputs are
// left out: foff, avail and have together (have is not read then), row0 and nrow together; with all of them null the
// question alone is answered (asked first: a push that does not fit leaves the mailbox alone).
inline bool chunk_rows(int U, int ncl, int64_t cluster_rows, const int32_t* counts, const int32_t* have, int64_t* foff, int32_t* avail,
                       uint32_t* row0, uint32_t* nrow) {
  bool fit = true;
  for (int c = 0; c < ncl; ++c) {
    const int64_t first = (int64_t)c * cluster_rows;
    int64_t pos = first;
    for (int u = c; u < U; pos += counts[u], u += ncl)
      if (foff) { foff[u] = pos - have[u]; avail[u] = have[u] + counts[u]; }
    fit = fit && pos - first <= cluster_rows;
    if (row0) { row0[c] = (uint32_t)first; nrow[c] = (uint32_t)(pos - first); }
  }
  return fit;
}

#endif  // UIS_PUSH_LAYOUT_H_
