// push_layout_main.cpp -- the two layouts and the chunk rows of uisrnn_amd/csrc/uis_push_layout.h.  Stand-alone: built
// with the host compiler (tests/test_push_layout_host.py builds it plain and with -fsanitize=address,undefined), no
// HIP, no library.
//
//   ChunkLayout: U of 1, 3, 4, 5 (U * 4 is a multiple of 16 only for 4) x F of 1, 17 x host frames / tensors, against
//   the formulas the push used before the header existed, restated here for every U; alignment (16 bytes for the
//   frames of an even U, 8 for an odd one: as it was); what travels;
//   MailboxLayout: U of 1, ncl, ncl + 1, 64: every region 128-byte aligned, in the order the launch was given them
//   all along, none overlapping; cluster_rows / cap_frames / hdr_stride against the expressions restated here;
//   chunk rows: counts with zeros, a window that holds frames, U no multiple of ncl: the per-cluster fill and the linear
//   one agree on avail, cluster c starts at c * cluster_rows, nrow[c] sums its counts, the rows are the ones the fill
//   loops of the push gave; a share of exactly cluster_rows fits, one row more does not.
// Exit status 0 iff all of that holds.

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "uis_push_layout.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what, const std::string& detail = "") {
  if (ok) return;
  ++failures;
  if (failures <= 20) fprintf(stderr, "FAILED: %s (%s)\n", what, detail.c_str());
}

const size_t kCtlWords = 832;       // (UIS_PM_CTL_WORDS)
const int64_t kRowsMax = 24 * 16 * 6;  // (UIS_RES_HEAD_TILES * 16 * 6: the one-launch kernel's row list)
const size_t kTableStride = 32;  // (sizeof(IngestBlock): two 16-byte words)

void chunk_layouts() {
  for (int U : {1, 3, 4, 5})
    for (int64_t F : {(int64_t)1, (int64_t)17})
      for (int D : {256, 37})
        for (bool tensors : {false, true}) {
          const std::string at = "U " + std::to_string(U) + " F " + std::to_string(F) + " D " + std::to_string(D) + (tensors ? " tensors" : " host");
          const ChunkLayout l(U, F, D, tensors, kTableStride);
          // the push's own arithmetic, as it stood before the header existed: the ground truth, for every U
          const size_t lead = tensors ? (size_t)U * kTableStride : 0;
          const size_t hdr = lead + (size_t)U * 8 + (((size_t)U * 4 + 15) & ~(size_t)15);
          const size_t need = hdr + (size_t)F * D * 4;
          const size_t staged = tensors ? hdr : need;
          expect(l.o_foff == lead, "the table in front, and foff behind it", at);
          expect(l.o_avail == lead + (size_t)U * 8, "avail", at);
          expect(l.o_frames == hdr, "frames", at);
          expect(l.total_bytes == need, "total", at);
          expect(l.travel_bytes == staged, "travel", at);
          // what the kernels rely on
          expect(l.o_foff % 8 == 0, "foff is 8-byte aligned", at);
          expect(l.o_avail % 4 == 0, "avail is 4-byte aligned", at);
          // The frame area lies directly behind avail padded to 16 bytes.  That makes it 16-byte aligned where U * 8 is a
          // multiple of 16: for an even U.  For an odd U it sits on an 8-byte boundary -- a finding of this test, on
          // record in DESIGN.md section 32; the layout is kept as it was, so the residue is asserted as it is.
          const size_t avail_end = l.o_avail + (size_t)U * 4;
          expect(l.o_frames == l.o_avail + ((avail_end - l.o_avail + 15) & ~(size_t)15), "the frame area is directly behind the padded avail", at);
          expect(l.o_frames % 16 == (U % 2 ? 8u : 0u), "the frame area is 16-byte aligned for an even U, 8 bytes off for an odd one", at);
          expect(l.o_frames % 8 == 0, "the frame area is 8-byte aligned", at);
          expect(l.travel_bytes == (tensors ? l.o_frames : l.o_frames + (size_t)F * D * 4), "what the one H2D carries", at);
          if (U == 4) expect(l.o_frames == avail_end, "U = 4 needs no pad", at);
          // the views
          std::vector<char> block(l.total_bytes);
          expect((char*)uis_block_at<int64_t>(block.data(), l.o_foff) == block.data() + l.o_foff &&
                     (char*)uis_block_at<float>(block.data(), l.o_frames) == block.data() + l.o_frames, "the view", at);
        }
}

void mailbox_layouts() {
  const int B = 10, D = 256;
  const int64_t max_frames = 100;
  for (int ncl : {1, 3, 8})
    for (int U : {1, ncl, ncl + 1, 64}) {
      const std::string at = "U " + std::to_string(U) + " ncl " + std::to_string(ncl);
      const MailboxLayout l = MailboxLayout(U, B, D, max_frames, ncl, kCtlWords, kRowsMax);
      // uis_stream_begin's expressions, as they stood (UIS_RES_HEAD_TILES * 16 * 6 = 24 * 16 * 6 rows is the cap)
      const int64_t share = ((U + ncl - 1) / ncl) * 16;
      const int64_t cluster_rows = std::min<int64_t>((share + 31) / 32 * 32, (int64_t)24 * 16 * 6);
      expect(l.cluster_rows == cluster_rows, "cluster_rows", at);
      expect(l.cap_frames == cluster_rows * ncl, "cap_frames", at);
      expect(l.hdr_stride == ((((size_t)U * 12) + 127) & ~(size_t)127), "hdr_stride", at);
      expect(l.hdr_stride >= (size_t)U * 12 && l.hdr_stride % 128 == 0, "a cluster's header copy fits its stride", at);
      // the regions in the launch's order, with their sizes
      const size_t start[9] = {0, l.o_foff, l.o_avail, l.o_lab_off, l.o_scores, l.o_beam_scores, l.o_overflow, l.o_frames, l.o_labels};
      const size_t bytes[9] = {(size_t)832 * 4, (size_t)U * 8, (size_t)U * 4, (size_t)U * 8, (size_t)U * 4, (size_t)U * B * 4, (size_t)U * 4,
                               (size_t)l.cap_frames * D * 4, (size_t)U * (size_t)max_frames * 4};
      for (int i = 0; i < 9; ++i) {
        expect(start[i] % 128 == 0, "a region is 128-byte aligned", at + " region " + std::to_string(i));
        if (i > 0) {
          expect(start[i] >= start[i - 1] + bytes[i - 1], "a region starts behind its predecessor", at + " region " + std::to_string(i));
          expect(start[i] - (start[i - 1] + bytes[i - 1]) < 128, "a region starts at the next 128-byte line", at + " region " + std::to_string(i));
        }
      }
      expect(l.total == start[8] + bytes[8], "total", at);
      std::vector<unsigned char> block(l.total);
      void* base = block.data();
      expect((unsigned char*)uis_block_at<int32_t>(base, l.o_labels) == block.data() + l.o_labels, "the view", at);
    }
  // the cap: 2304 rows a cluster, whatever the session's size
  expect(MailboxLayout(64 * 200, B, D, 4, 1, kCtlWords, kRowsMax).cluster_rows == 24 * 16 * 6, "cluster_rows is capped");
}

void chunk_rows_cases() {
  struct Case { int U, ncl; std::vector<int32_t> counts, have; };
  const std::vector<Case> cases = {
      {1, 1, {3}, {0}},
      {5, 2, {2, 0, 1, 0, 4}, {7, 0, 3, 9, 1}},       // zeros, a window that holds frames, U no multiple of ncl
      {7, 3, {0, 0, 0, 5, 0, 0, 1}, {1, 2, 3, 4, 5, 6, 7}},
      {8, 8, {1, 1, 1, 1, 1, 1, 1, 1}, {0, 0, 0, 0, 0, 0, 0, 0}},
      {9, 4, {16, 0, 3, 1, 0, 2, 16, 5, 16}, {100, 0, 0, 50, 2, 0, 1, 0, 31}},
  };
  for (size_t i = 0; i < cases.size(); ++i) {
    const Case& c = cases[i];
    const std::string at = "case " + std::to_string(i);
    const int64_t cluster_rows = MailboxLayout(c.U, 10, 256, 1000, c.ncl, kCtlWords, kRowsMax).cluster_rows;
    std::vector<int64_t> foff_lin(c.U, -99), foff_cl(c.U, -99);
    std::vector<int32_t> avail_lin(c.U, -99), avail_cl(c.U, -99);
    std::vector<uint32_t> row0(c.ncl, 99), nrow(c.ncl, 99);
    ::chunk_rows(c.U, 1, 0, c.counts.data(), c.have.data(), foff_lin.data(), avail_lin.data(), nullptr, nullptr);  // (the ordinary push)
    // (the question alone first: nothing is written, and both calls give the same answer)
    expect(::chunk_rows(c.U, c.ncl, cluster_rows, c.counts.data(), c.have.data(), nullptr, nullptr, nullptr, nullptr), "the case fits", at);
    expect(::chunk_rows(c.U, c.ncl, cluster_rows, c.counts.data(), c.have.data(), foff_cl.data(), avail_cl.data(), row0.data(), nrow.data()),
           "the case fits, asked with the fill", at);
    expect(avail_lin == avail_cl, "both fills give the same avail", at);
    // the linear fill: the first new frame of utterance u (step have[u]) is the row behind its predecessors' frames
    int64_t pos = 0;
    for (int u = 0; u < c.U; ++u) {
      expect(foff_lin[u] + c.have[u] == pos, "linear: the row of the first new frame", at);
      expect(avail_lin[u] == c.have[u] + c.counts[u], "avail = have + counts", at);
      pos += c.counts[u];
    }
    // the per-cluster fill: cluster k owns utterances k, k + ncl, ... from the start of its fixed range
    for (int k = 0; k < c.ncl; ++k) {
      expect(row0[k] == (uint32_t)(k * cluster_rows), "a cluster's rows start at its fixed range", at);
      int64_t p = (int64_t)k * cluster_rows, sum = 0;
      for (int u = k; u < c.U; u += c.ncl) {
        expect(foff_cl[u] + c.have[u] == p, "clustered: the row of the first new frame", at);
        p += c.counts[u];
        sum += c.counts[u];
      }
      expect(nrow[k] == (uint32_t)sum, "nrow sums the cluster's counts", at);
      expect(row0[k] + nrow[k] <= (uint32_t)((k + 1) * cluster_rows), "a cluster stays inside its range", at);
    }
  }
  // a share of exactly cluster_rows fits, one row more does not (cluster 1 of 2 owns utterances 1 and 3)
  const int64_t rows = MailboxLayout(4, 10, 256, 1000, 2, kCtlWords, kRowsMax).cluster_rows;
  expect(rows == 32, "two utterances a cluster: 32 rows");
  int32_t counts[4] = {0, 20, 5, 12};
  const int32_t none[4] = {0, 0, 0, 0};
  const auto chunk_rows_fit = [&](int U, int ncl, int64_t cluster_rows, const int32_t* n) {
    return ::chunk_rows(U, ncl, cluster_rows, n, none, nullptr, nullptr, nullptr, nullptr);
  };
  expect(chunk_rows_fit(4, 2, rows, counts), "a share of exactly cluster_rows fits");
  counts[3] = 13;
  expect(!chunk_rows_fit(4, 2, rows, counts), "one row more does not");
  counts[3] = 12; counts[0] = 28;
  expect(!chunk_rows_fit(4, 2, rows, counts), "nor in the first cluster");
}

}  // namespace

int main() {
  chunk_layouts();
  mailbox_layouts();
  chunk_rows_cases();
  if (failures) {
    fprintf(stderr, "push_layout: %d check(s) failed\n", failures);
    return 1;
  }
  printf("push_layout: ok\n");
  return 0;
}
