// blob_check_main.cpp -- the host validator of uisrnn_amd/csrc/uis_blob.h against damaged blobs.  Stand-alone: built
// with the host compiler (tests/test_migrate_host.py adds -fsanitize=address,undefined), no HIP, no library.
//
// A well-formed blob is built here; the validator must accept it and refuse
//   every truncation (each prefix length, checked through a heap copy of exactly that size, so that a read past the
//   bytes given is the sanitizer's to report), one byte more, one byte less;
//   every single 32-bit word xor-ed with each of a few patterns (the checksum, the magic, the end word);
//   hostile values in every word that steers an address or a loop bound, with the blob SEALED AGAIN afterwards, so
//   that the structural checks and not the checksum have to catch them;
//   another model, numerics version or beam (UIS_BLOB_MISMATCH).
// Exit status 0 iff all of that holds.

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "uis_blob.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what, long detail = -1) {
  if (ok) return;
  ++failures;
  if (failures <= 20) fprintf(stderr, "FAILED: %s (%ld)\n", what, detail);
}

const UisBlobShape kShape = {3u, 3, 5, 16, 7, 16, 2, 0, 0, 0x1234567890abcdefull};

// beam 3, two live ranks with K = 2 and 3 over n = 4 slots, N = 5 window frames (15 record words: a pad of one)
std::vector<char> make_blob(UisBlobLayout* lay) {
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
  sc.committed = 40; sc.N = N; sc.live = live; sc.n = n; sc.lists = lists; sc.win_score = 12.5f;
  memcpy(b.data() + l.scalars, &sc, sizeof(sc));
  const UisBlobRank ranks[2] = {{2, 1, 9, 3.25f}, {3, 0, 11, 4.5f}};
  memcpy(b.data() + l.ranks, ranks, sizeof(ranks));
  const int32_t lst[10] = {0, 2, /*blk*/ 4, 5, /*rank 1*/ 0, 1, 3, /*blk*/ 4, 6, 1};
  memcpy(b.data() + l.lists, lst, sizeof(lst));
  const int32_t cnt[4] = {20, 3, 17, 1};
  memcpy(b.data() + l.cnt, cnt, sizeof(cnt));
  for (int64_t i = l.mean; i < l.records; i += 4) { const float v = (float)(i % 97) * 0.5f; memcpy(b.data() + i, &v, 4); }
  for (int i = 0; i < N * B; ++i) { const uint32_t v = (uint32_t)(i % 3) | (uint32_t)(i % B) << 16; memcpy(b.data() + l.records + 4 * i, &v, 4); }
  uis_blob_seal(b.data(), l);
  *lay = l;
  return b;
}

// through a heap copy of exactly `bytes` bytes: a read past the end is out of bounds for the sanitizer
int validate(const char* data, int64_t bytes, const UisBlobShape* expect_shape) {
  char* copy = static_cast<char*>(malloc(bytes > 0 ? (size_t)bytes : 1));
  if (bytes > 0) memcpy(copy, data, (size_t)bytes);
  UisBlobInfo info;
  const char* why = nullptr;
  const int rc = uis_blob_validate(copy, bytes, expect_shape, &info, &why);
  free(copy);
  if (rc != UIS_BLOB_OK && (!why || !*why)) { ++failures; fprintf(stderr, "FAILED: a refusal without a reason\n"); }
  return rc;
}

void put32(std::vector<char>& b, int64_t at, int32_t v) { memcpy(b.data() + at, &v, 4); }
void put64(std::vector<char>& b, int64_t at, int64_t v) { memcpy(b.data() + at, &v, 8); }

// the trailer's hash again, over the mutated bytes: the checksum is right and only the structure is wrong
void reseal(std::vector<char>& b, const UisBlobLayout& orig) {
  const uint64_t tr[2] = {uis_blob_hash(b.data(), (size_t)orig.trailer, 0), UIS_BLOB_END};
  memcpy(b.data() + orig.trailer, tr, 16);
}

}  // namespace

int main() {
  UisBlobLayout l;
  const std::vector<char> good = make_blob(&l);
  const int64_t total = l.total;
  expect(validate(good.data(), total, &kShape) == UIS_BLOB_OK, "the original is accepted");
  expect(validate(good.data(), total, nullptr) == UIS_BLOB_OK, "the original is accepted without a shape");
  expect(uis_blob_validate(nullptr, total, &kShape, nullptr, nullptr) == UIS_BLOB_MALFORMED, "a null blob");
  // ---- truncations and a byte too many
  for (int64_t bytes = 0; bytes < total; ++bytes)
    expect(validate(good.data(), bytes, &kShape) == UIS_BLOB_MALFORMED, "a truncation is refused", (long)bytes);
  {
    std::vector<char> longer(good);
    longer.push_back(0);
    expect(validate(longer.data(), total + 1, &kShape) == UIS_BLOB_MALFORMED, "one byte more");
  }
  expect(validate(good.data(), -5, &kShape) == UIS_BLOB_MALFORMED, "a negative size");
  // ---- single-word mutations, not sealed again
  const uint32_t patterns[] = {1u, 0x80000000u, 0xffffffffu, 0x00010000u};
  for (int64_t at = 0; at + 4 <= total; at += 4)
    for (uint32_t p : patterns) {
      std::vector<char> b(good);
      uint32_t w;
      memcpy(&w, b.data() + at, 4);
      w ^= p;
      memcpy(b.data() + at, &w, 4);
      expect(validate(b.data(), total, &kShape) != UIS_BLOB_OK, "a flipped word is refused", (long)at);
    }
  // ---- hostile structure under a valid checksum
  struct Word { int64_t at; const char* what; };
  const int64_t S = l.scalars, R = l.ranks, L = l.lists;
  const Word words[] = {
      {16, "B"}, {20, "D"}, {24, "Dp"}, {28, "H"}, {32, "Hp"}, {36, "depth"},
      {S + 8, "N"}, {S + 12, "live"}, {S + 16, "n"}, {S + 20, "lists"},
      {R + 0, "rank 0 K"}, {R + 4, "rank 0 last"}, {R + 8, "rank 0 sum"}, {R + 16, "rank 1 K"}, {R + 20, "rank 1 last"},
      {L + 0, "rank 0 slot 0"}, {L + 4, "rank 0 slot 1"}, {L + 8, "rank 0 blk 0"}, {L + 16, "rank 1 slot 0"}, {L + 36, "rank 1 blk 2"},
      {l.cnt + 0, "cnt 0"}, {l.cnt + 12, "cnt 3"},
  };
  const int32_t hostile[] = {-1, -2147483647 - 1, 2147483647, 0x7fffff00, 1 << 20, 4097, 257};
  for (const Word& w : words)
    for (int32_t v : hostile) {
      std::vector<char> b(good);
      int32_t old;
      memcpy(&old, b.data() + w.at, 4);
      if (old == v) continue;
      put32(b, w.at, v);
      reseal(b, l);
      expect(validate(b.data(), total, &kShape) != UIS_BLOB_OK, w.what, (long)v);
    }
  {
    const int64_t hostile64[] = {-1, 0x7fffff00ll, (int64_t)1 << 62, INT64_MIN};
    for (int64_t v : hostile64) {
      std::vector<char> b(good);
      put64(b, S, v);   // committed
      reseal(b, l);
      expect(validate(b.data(), total, &kShape) != UIS_BLOB_OK, "committed", (long)v);
      b = good;
      put64(b, 56, v);  // total_bytes
      reseal(b, l);
      expect(validate(b.data(), total, &kShape) != UIS_BLOB_OK, "total_bytes", (long)v);
    }
  }
  {  // zero values where one is the least; last = -1 with K > 0; slot index = n; a non-zero pad; a bad end word
    const struct { int64_t at; int32_t v; const char* what; } cases[] = {
        {S + 12, 0, "live = 0"}, {S + 12, 4, "live = B + 1"}, {16, 0, "B = 0"}, {36, 0, "depth = 0"}, {36, 9, "depth = 9"},
        {R + 4, -1, "last = -1 at K = 2"}, {R + 4, 2, "last = K"}, {L + 4, 4, "slot = n"}, {l.cnt + 4, 0, "cnt = 0"},
        {L + 40, 1, "the lists' pad"}, {l.records + 60, 1, "the records' pad"}, {S + 28, 1, "the reserved word"},
        {R + 8, 10, "sum off by one"}, {12, 2, "look_ahead 2"}, {4, 2, "format 2"},
    };
    for (const auto& c : cases) {
      std::vector<char> b(good);
      put32(b, c.at, c.v);
      reseal(b, l);
      expect(validate(b.data(), total, &kShape) != UIS_BLOB_OK, c.what);
    }
    std::vector<char> b(good);
    put64(b, l.trailer + 8, 0);
    expect(validate(b.data(), total, &kShape) != UIS_BLOB_OK, "a bad end word");
  }
  // ---- a well-formed blob of somebody else
  {
    UisBlobShape other = kShape;
    other.model_hash ^= 1;
    expect(validate(good.data(), total, &other) == UIS_BLOB_MISMATCH, "another model's parameters");
    other = kShape; other.B = 4;
    expect(validate(good.data(), total, &other) == UIS_BLOB_MISMATCH, "another beam");
    other = kShape; other.numerics = 4;
    expect(validate(good.data(), total, &other) == UIS_BLOB_MISMATCH, "another numerics version");
    other = kShape; other.Hp = 32;
    expect(validate(good.data(), total, &other) == UIS_BLOB_MISMATCH, "another padded shape");
  }
  if (failures) {
    fprintf(stderr, "blob_check: %d failures\n", failures);
    return 1;
  }
  printf("blob_check: ok (%lld bytes)\n", (long long)total);
  return 0;
}
