// blob_turn_main.cpp -- uisrnn_amd/csrc/uis_blob.h on blobs whose last-label words carry a run (bits 16 .. 30): the
// host validator and uis_blob_last_word, the one function uis_stream_import normalises a word with.  Stand-alone: built
// with the host compiler (tests/test_turn_session_host.py also adds -fsanitize=address,undefined), no HIP, no library.
//
//   uis_blob_last_word over a word of every kind -- no label, a bare label, a run below / at / above m, the largest
//   label and run the word holds -- against m in {0, 1, 2, 3, 32767}, each against the rule written out;
//   a blob without runs validates as before, with max_run 0;
//   a blob with runs validates, max_run is the largest, max_K and max_tag are what they were;
//   the damaged blobs stay malformed: last = K and last = -1 at K = 2 (bare and under run bits), a run beside "no
//   label", a word with K = 0 that is not exactly -1, ranks of which one has a run and another has none.
// With a path as its argument it writes the accepted blob with runs there.
// Exit status 0 iff all of that holds.

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "uis_blob.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what) {
  if (ok) return;
  ++failures;
  fprintf(stderr, "FAILED: %s\n", what);
}

const UisBlobShape kShape = {3u, 3, 5, 16, 7, 16, 2, 0, 0, 0x1234567890abcdefull};

int32_t word(int32_t label, int32_t run) { return label | (int32_t)((uint32_t)run << 16); }

// beam 3, two live ranks with K = K0 and 3 over n = 4 slots, N = 5 window frames after `committed`; last0 / last1: the
// ranks' last-label words as given (K0 = 0: rank 0 has no cluster, and n = 3)
std::vector<char> make_blob(int64_t committed, int32_t K0, int32_t last0, int32_t last1) {
  const int B = kShape.B, Dp = kShape.Dp, Hp = kShape.Hp, depth = kShape.depth, N = 5, live = 2, n = K0 == 2 ? 4 : 3, lists = K0 + 3;
  const UisBlobLayout l = uis_blob_layout(B, Dp, Hp, depth, N, live, n, lists);
  std::vector<char> b((size_t)l.total, 0);
  UisBlobHeader hd;
  memset(&hd, 0, sizeof(hd));
  hd.magic = UIS_BLOB_MAGIC; hd.format = UIS_BLOB_FORMAT; hd.numerics = kShape.numerics; hd.look_ahead = 1;
  hd.B = B; hd.D = kShape.D; hd.Dp = Dp; hd.H = kShape.H; hd.Hp = Hp; hd.depth = depth;
  hd.hid_seg = kShape.hid_seg; hd.hid_seg_p = kShape.hid_seg_p; hd.model_hash = kShape.model_hash;
  memcpy(b.data(), &hd, sizeof(hd));
  UisBlobScalars sc;
  memset(&sc, 0, sizeof(sc));
  sc.committed = committed; sc.N = N; sc.live = live; sc.n = n; sc.lists = lists; sc.win_score = 12.5f;
  memcpy(b.data() + l.scalars, &sc, sizeof(sc));
  const UisBlobRank ranks[2] = {{K0, last0, K0 == 2 ? 3 : 0, 3.25f}, {3, last1, 4, 4.5f}};
  memcpy(b.data() + l.ranks, ranks, sizeof(ranks));
  std::vector<int32_t> lst;
  if (K0 == 2) { lst.insert(lst.end(), {0, 2, /*blk*/ 1, 2}); }
  lst.insert(lst.end(), {0, 1, n - 1, /*blk*/ 2, 1, 1});
  memcpy(b.data() + l.lists, lst.data(), lst.size() * 4);
  const int32_t cnt[4] = {2, 3, 1, 1};
  memcpy(b.data() + l.cnt, cnt, (size_t)n * 4);
  for (int64_t i = l.mean; i < l.records; i += 4) { const float v = (float)(i % 97) * 0.5f; memcpy(b.data() + i, &v, 4); }
  for (int i = 0; i < N * B; ++i) { const uint32_t v = (uint32_t)(i % 3) | (uint32_t)(i % B) << 16; memcpy(b.data() + l.records + 4 * i, &v, 4); }
  uis_blob_seal(b.data(), l);
  return b;
}

int check(const std::vector<char>& b, UisBlobInfo* info = nullptr) {
  const char* why = nullptr;
  return uis_blob_validate(b.data(), (int64_t)b.size(), &kShape, info, &why);
}

// the rule of include/uisrnn_hip.h, written out
int32_t rule(int32_t label, int32_t run, int32_t m) {
  if (label < 0) return -1;
  if (m < 2) return label;
  if (run == 0) return word(label, m);
  return word(label, run < m ? run : m);
}

}  // namespace

int main(int argc, char** argv) {
  // ---- uis_blob_last_word
  const int32_t ms[5] = {0, 1, 2, 3, 32767};
  const int32_t labels[5] = {0, 1, 7, 4095, 32767};
  const int32_t runs[8] = {0, 1, 2, 3, 4, 5, 32766, 32767};
  for (int32_t m : ms) {
    expect(uis_blob_last_word(-1, m) == -1, "no label stays -1");
    for (int32_t label : labels)
      for (int32_t run : runs) {
        const int32_t got = uis_blob_last_word(word(label, run), m);
        expect(got == rule(label, run, m), "uis_blob_last_word is the rule");
        expect(uis_blob_last_label(got) == label, "the label survives");
        expect(got >= 0 && (m < 2 ? uis_blob_last_run(got) == 0 : (uis_blob_last_run(got) >= 1 && uis_blob_last_run(got) <= m)),
               "the run is 0 without a rule and in [1, m] under one");
        expect(uis_blob_last_word(got, m) == got, "normalising twice changes nothing");
      }
  }
  expect(uis_blob_last_word(word(2, 0), 3) == word(2, 3), "a word without a run gets run m");
  expect(uis_blob_last_word(word(2, 5), 3) == word(2, 3), "a run above m is clamped");
  expect(uis_blob_last_word(word(2, 2), 3) == word(2, 2), "a run below m is kept");
  expect(uis_blob_last_word(word(2, 2), 0) == 2 && uis_blob_last_word(word(2, 2), 1) == 2, "m < 2 gives the bare label");
  expect(uis_blob_last_label(-1) == -1 && uis_blob_last_label(word(4095, 32767)) == 4095 && uis_blob_last_run(word(4095, 32767)) == 32767,
         "the word's two fields");

  // ---- the validator
  UisBlobInfo info;
  memset(&info, 0, sizeof(info));
  expect(check(make_blob(40, 2, 1, 0), &info) == UIS_BLOB_OK && info.max_run == 0 && info.max_K == 3 && info.max_tag == 0,
         "a blob without runs validates, max_run 0");
  const std::vector<char> with_runs = make_blob(40, 2, word(1, 2), word(0, 5));
  expect(check(with_runs, &info) == UIS_BLOB_OK && info.max_run == 5 && info.max_K == 3 && info.max_tag == 0,
         "a blob with runs validates, max_run the largest");
  expect(check(make_blob(0, 2, word(1, 32767), word(2, 1)), &info) == UIS_BLOB_OK && info.max_run == 32767,
         "a run is not bounded by the stream: a word that arrived without one holds the slot's value");
  expect(check(make_blob(40, 0, -1, word(2, 3)), &info) == UIS_BLOB_OK && info.max_run == 3, "a rank without clusters holds -1");
  // damaged
  expect(check(make_blob(40, 2, 2, 0)) == UIS_BLOB_MALFORMED, "last = K stays malformed");
  expect(check(make_blob(40, 2, -1, 0)) == UIS_BLOB_MALFORMED, "last = -1 at K = 2 stays malformed");
  expect(check(make_blob(40, 2, word(2, 3), word(0, 1))) == UIS_BLOB_MALFORMED, "last = K under run bits is malformed");
  expect(check(make_blob(40, 2, word(0xffff, 3), word(0, 1))) == UIS_BLOB_MALFORMED, "a run beside 'no label' is malformed");
  expect(check(make_blob(40, 2, (int32_t)0x80010001u, word(0, 1))) == UIS_BLOB_MALFORMED, "a negative word is malformed");
  expect(check(make_blob(40, 0, 0, 0)) == UIS_BLOB_MALFORMED, "K = 0 with last = 0 is malformed");
  expect(check(make_blob(40, 0, word(0xffff, 0), 0)) == UIS_BLOB_MALFORMED, "K = 0 with a 16-bit -1 is not exactly -1");
  expect(check(make_blob(40, 0, word(0xffff, 2), word(0, 1))) == UIS_BLOB_MALFORMED, "K = 0 with run bits is malformed");
  expect(check(make_blob(40, 2, word(1, 16), 0)) == UIS_BLOB_MALFORMED, "a run in one rank and none in another is malformed");
  expect(check(make_blob(40, 2, 1, word(0, 16))) == UIS_BLOB_MALFORMED, "... whichever rank comes first");

  if (argc > 1) {
    FILE* f = fopen(argv[1], "wb");
    expect(f != nullptr, "the output file opens");
    if (f) {
      expect(fwrite(with_runs.data(), 1, with_runs.size(), f) == with_runs.size(), "the blob is written");
      fclose(f);
    }
  }
  if (failures) return 1;
  printf("blob_turn: ok\n");
  return 0;
}
