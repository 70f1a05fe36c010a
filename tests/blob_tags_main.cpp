// blob_tags_main.cpp -- the host validator of uisrnn_amd/csrc/uis_blob.h on blobs whose block-count words carry speaker
// tags (bits 24 .. 30).  Stand-alone: built with the host compiler (tests/test_known_session_host.py also adds
// -fsanitize=address,undefined), no HIP, no library.
//
// A well-formed blob is built here, without tags and with them; the validator must
//   accept the untagged blob as before, with max_tag 0;
//   accept distinct tags within a rank -- also the same tag in two ranks, also tag 127 -- and report the largest;
//   refuse a tag bound twice in one rank;
//   refuse a tagged blob at committed + N = 2^24, and accept the untagged one there and the tagged one a frame earlier;
//   refuse a rank whose sum only adds up when the tags are counted in.
// With a path as its argument it writes the accepted tagged blob there (the Python helper reads it).
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

// beam 3, two live ranks with K = 2 and 3 over n = 4 slots, N = 5 window frames; tags[i]: the tag of list entry i
// (rank 0's two clusters, then rank 1's three); sums: what the ranks claim
std::vector<char> make_blob(int64_t committed, const int tags[5], int32_t sum0, int32_t sum1) {
  const int B = kShape.B, Dp = kShape.Dp, Hp = kShape.Hp, depth = kShape.depth, N = 5, live = 2, n = 4, lists = 5;
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
  const UisBlobRank ranks[2] = {{2, 1, sum0, 3.25f}, {3, 0, sum1, 4.5f}};
  memcpy(b.data() + l.ranks, ranks, sizeof(ranks));
  const int32_t counts[5] = {4, 5, 4, 6, 1};
  int32_t w[5];
  for (int i = 0; i < 5; ++i) w[i] = counts[i] | (int32_t)((uint32_t)tags[i] << UIS_BLOB_BLK_TAG_SHIFT);
  const int32_t lst[10] = {0, 2, /*blk*/ w[0], w[1], /*rank 1*/ 0, 1, 3, /*blk*/ w[2], w[3], w[4]};
  memcpy(b.data() + l.lists, lst, sizeof(lst));
  const int32_t cnt[4] = {20, 3, 17, 1};
  memcpy(b.data() + l.cnt, cnt, sizeof(cnt));
  for (int64_t i = l.mean; i < l.records; i += 4) { const float v = (float)(i % 97) * 0.5f; memcpy(b.data() + i, &v, 4); }
  for (int i = 0; i < N * B; ++i) { const uint32_t v = (uint32_t)(i % 3) | (uint32_t)(i % B) << 16; memcpy(b.data() + l.records + 4 * i, &v, 4); }
  uis_blob_seal(b.data(), l);
  return b;
}

// through a heap copy of exactly the blob's size: a read past the end is out of bounds for the sanitizer
int validate(const std::vector<char>& blob, UisBlobInfo* info, const char** why) {
  char* copy = static_cast<char*>(malloc(blob.size()));
  memcpy(copy, blob.data(), blob.size());
  memset(info, 0x5a, sizeof(*info));
  const int rc = uis_blob_validate(copy, (int64_t)blob.size(), &kShape, info, why);
  free(copy);
  return rc;
}

}  // namespace

int main(int argc, char** argv) {
  UisBlobInfo info;
  const char* why = "";
  const int none[5] = {0, 0, 0, 0, 0};
  const int distinct[5] = {9, 0, 3, 9, 127};        // tag 9 in both ranks, on different indices: the ranks bind on their own
  const int twice[5] = {0, 0, 3, 0, 3};             // rank 1 binds tag 3 to two clusters
  const int64_t edge = ((int64_t)1 << 24) - 5;      // committed + N = 2^24

  // ---- untagged: as before
  expect(validate(make_blob(40, none, 9, 11), &info, &why) == UIS_BLOB_OK, "an untagged blob is accepted");
  expect(info.max_tag == 0 && info.max_K == 3, "an untagged blob reports max_tag 0");
  // ---- distinct tags
  const std::vector<char> tagged = make_blob(40, distinct, 9, 11);
  expect(validate(tagged, &info, &why) == UIS_BLOB_OK, "a blob with distinct tags is accepted");
  expect(info.max_tag == 127, "the largest tag is reported");
  const int small[5] = {0, 2, 1, 0, 0};
  expect(validate(make_blob(40, small, 9, 11), &info, &why) == UIS_BLOB_OK && info.max_tag == 2, "max_tag is the maximum over the ranks");
  // ---- a tag bound twice in one rank
  expect(validate(make_blob(40, twice, 9, 11), &info, &why) == UIS_BLOB_MALFORMED, "a tag bound twice is refused");
  expect(strstr(why, "a tag bound twice") != nullptr, "... in those words");
  // ---- the 2^24 bound
  expect(validate(make_blob(edge, distinct, 9, 11), &info, &why) == UIS_BLOB_MALFORMED, "a tagged blob at 2^24 frames is refused");
  expect(strstr(why, "2^24") != nullptr, "... in those words");
  expect(validate(make_blob(edge, none, 9, 11), &info, &why) == UIS_BLOB_OK, "an untagged blob at 2^24 frames is accepted");
  expect(validate(make_blob(edge - 1, distinct, 9, 11), &info, &why) == UIS_BLOB_OK, "a tagged blob one frame below 2^24 is accepted");
  // ---- sums: the counts alone must add up
  const int32_t unmasked0 = 9 + (9 << 24);
  expect(validate(make_blob(((int64_t)1 << 30), none, 9, 11), &info, &why) == UIS_BLOB_OK, "(a long untagged stream is a valid blob)");
  expect(validate(make_blob(40, distinct, unmasked0, 11), &info, &why) == UIS_BLOB_MALFORMED, "a sum that only adds up unmasked is refused");
  expect(strstr(why, "do not add up") != nullptr, "... in those words");
  expect(validate(make_blob(40, distinct, 9, 12), &info, &why) == UIS_BLOB_MALFORMED, "a wrong masked sum is refused");

  if (argc > 1) {
    FILE* f = fopen(argv[1], "wb");
    if (!f || fwrite(tagged.data(), 1, tagged.size(), f) != tagged.size()) { fprintf(stderr, "cannot write %s\n", argv[1]); return 2; }
    fclose(f);
  }
  if (failures) return 1;
  printf("blob_tags: ok\n");
  return 0;
}
