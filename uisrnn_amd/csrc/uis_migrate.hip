// uis_migrate.hip -- uis_stream_export / uis_stream_import: one utterance of a live session as a blob of bytes, and
// back into a slot that has received nothing -- of this session or of another one, another handle, device or process.
//
// Between two pushes an utterance is its tables (uis_prime.hip's header comment names them and who reads them again):
// utt_step, overflow, beam_n, the beam tables of the parity of its window frame count N, the pool slots its live
// hypotheses name, its bp rows [0, N), and three host words: have, committed, win_score.  No free list persists and
// every push rebuilds rows / counters / control words.  k_prime_commit writes "one hypothesis after P steps" into those
// tables; import writes "`live` hypotheses after N window steps", export reads the same back.  The blob's layout, its
// hash and the host's validator are uis_blob.h's.  No decode kernel changes and none runs here.
//
// Two kernels, templated on the direction, between launches, no floating point, no global atomics:
//   k_migrate_pack   one workgroup.  Export: a flag word per pool slot that a live rank names (S words in the scratch,
//                    not LDS: S = B * (max_clusters + 1) can exceed it), their prefix counts = the renumbering by
//                    ascending source slot (a function of the state alone; import puts blob slot j into pool slot j,
//                    so a second export reproduces the blob), the ranks' scalars, their compact slot / block lists,
//                    the slots' frame counts, and the control words the host reads (live, beam_n, overflow, n, list
//                    length).  Import: the same sections into ranks 0 .. live - 1 of the beam tables of parity N & 1,
//                    pool_cnt, beam_n = {live, 0}, utt_step = N, overflow = 0.  Export is verbatim; import passes each
//                    rank's last-label word through uis_blob_last_word against the target slot's minimum turn length
//   k_migrate_copy   workgroups [0, slot groups): the named slots' rows of pool_mean and pool_hid, 16 bytes per thread
//                    (rows are copied in the pool's padded / HidMap layout, never re-mapped); the rest: one tile of
//                    UIS_MIGRATE_TILE_WORDS record words each -- 16 bytes per thread where the utterance's records and
//                    the tile's place in the blob are both aligned, a scalar tail in the last tile, and the scalar path
//                    where the records are not (an odd beam at an odd max_frames on an odd utterance, k_commit_move's
//                    split).  Source and destination never overlap.
// The fresh-cluster source row of resident sessions (pool_hid + U * S * Hp) belongs to the session: not exported, not
// written.  Ranks from `live` on, slots from n on and record rows from N on of an imported utterance are dead memory
// that the stream defines before it reads it, as in a session that has just been opened.
//
// The order is the scaffold's (uis_stream.hip); this call's own: export's image is laid out for the largest blob the
// session can give (uis_stream_export_bound) and comes down in ONE copy with the control words in front; the host then
// closes the blob (header, scalars, zero pads, hash).  Import validates everything that steers an address or a loop
// bound on the host before session_enter, grows the prior tables like a commit (PriorTableGrowth) -- an utterance can
// arrive with `committed` far beyond what the target's tables reach --, and goes up in one copy.
//
// #included by uis_decoder.hip after uis_retire.hip.

namespace {

#define UIS_MIGRATE_THREADS 256
#define UIS_MIGRATE_TILE_WORDS 4096   // record words per workgroup of k_migrate_copy: four 16-byte accesses per thread
#define UIS_MIGRATE_SLOT_GROUPS 512   // at most this many workgroups share the slot rows
#define UIS_MIGRATE_CTL_BYTES 64      // export's control words, in front of the image

struct MigrateArgs {
  int u;                // the utterance
  int N, live, n, lists;  // import: from the validated blob; export: the kernels read the control words
  int slot_groups;
  int min_turn;         // import: the target slot's minimum turn length (uis_session_min_turn; below 2: no rule)
  int32_t* ctl;         // export: [0] live (0: overflow word set or beam empty) [1] beam_n [2] overflow [3] n [4] lists [5] N
  char* img;            // the blob's image in the scratch (16-byte aligned)
  int32_t* flags;       // [S] export: slot named by a live rank
  int32_t* map;         // [S] export: slot -> its number in the blob
  int32_t* slot_of;     // [S] export: blob slot -> pool slot
};

// words [0, count) of one tile: both pointers advance by whole tiles, so they keep their alignment mod 16
__device__ __forceinline__ void migrate_copy_words(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, long count) {
  const long tid = threadIdx.x;
  if (((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15u) == 0) {
    const long nvec = count >> 2;
    for (long i = tid; i < nvec; i += UIS_MIGRATE_THREADS) reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
    const long i = (nvec << 2) + tid;   // the scalar tail: up to three words
    if (i < count) dst[i] = src[i];
  } else {
    for (long i = tid; i < count; i += UIS_MIGRATE_THREADS) dst[i] = src[i];
  }
}

template <bool IMPORT>
__global__ __launch_bounds__(UIS_MIGRATE_THREADS) void k_migrate_pack(DevModel m, DecodeState st, MigrateArgs a) {
  __shared__ int s_K[256];      // (beam_size <= 256)
  __shared__ int s_off[257];    // where rank r's entries start in the lists
  __shared__ int s_wave[UIS_MIGRATE_THREADS / 64];
  const int tid = threadIdx.x, u = a.u;
  const int B = st.B, Kmax = st.Kmax, S = st.S;
  if (IMPORT) {
    const UisBlobLayout l = uis_blob_layout(B, m.Dp, m.Hp, m.depth, a.N, a.live, a.n, a.lists);
    const int par = a.N & 1;
    const size_t e = ((size_t)par * st.U + u) * B;
    const UisBlobRank* ranks = reinterpret_cast<const UisBlobRank*>(a.img + l.ranks);
    const int32_t* lists = reinterpret_cast<const int32_t*>(a.img + l.lists);
    const int32_t* cnt = reinterpret_cast<const int32_t*>(a.img + l.cnt);
    if (tid < a.live) {
      const UisBlobRank rk = ranks[tid];
      s_K[tid] = rk.K;
      st.beam_K[e + tid] = rk.K; st.beam_last[e + tid] = uis_blob_last_word(rk.last, a.min_turn); st.beam_sum[e + tid] = rk.sum; st.beam_score[e + tid] = rk.score;
    }
    __syncthreads();
    if (tid == 0) {
      int acc = 0;
      for (int r = 0; r < a.live; ++r) { s_off[r] = acc; acc += s_K[r]; }
    }
    __syncthreads();
    for (int r = 0; r < a.live; ++r) {
      const int K = s_K[r];
      const int32_t* src = lists + 2 * (size_t)s_off[r];
      for (int k = tid; k < K; k += UIS_MIGRATE_THREADS) {
        st.beam_slot[(e + r) * Kmax + k] = src[k];
        st.beam_blk[(e + r) * Kmax + k] = src[K + k];
      }
    }
    for (int j = tid; j < a.n; j += UIS_MIGRATE_THREADS) st.pool_cnt[(size_t)u * S + j] = cnt[j];
    if (tid == 0) {
      st.beam_n[(size_t)par * st.U + u] = a.live;
      st.beam_n[(size_t)(par ^ 1) * st.U + u] = 0;
      st.utt_step[u] = a.N;
      st.overflow[u] = 0;
    }
    return;
  }
  // ---- export
  const auto [N, T, par, nb, live, e, bp] = beam_view(st, u, EMPTY_WINDOW_KEEPS_BEAM);
  if (live == 0) {   // flagged in the overflow word, or the beam is empty: nothing to move
    if (tid == 0) { a.ctl[0] = 0; a.ctl[1] = nb; a.ctl[2] = st.overflow[u]; a.ctl[3] = 0; a.ctl[4] = 0; a.ctl[5] = (int32_t)N; }
    return;
  }
  for (int s = tid; s < S; s += UIS_MIGRATE_THREADS) a.flags[s] = 0;
  if (tid < live) {
    const int K = st.beam_K[e + tid];
    s_K[tid] = K < 0 ? 0 : (K > Kmax ? Kmax : K);
  }
  __syncthreads();
  if (tid == 0) {
    int acc = 0;
    for (int r = 0; r < live; ++r) { s_off[r] = acc; acc += s_K[r]; }
    s_off[live] = acc;
  }
  // ---- the slots the live ranks name (every writer stores the same word)
  for (int r = 0; r < live; ++r)
    for (int k = tid; k < s_K[r]; k += UIS_MIGRATE_THREADS) {
      const int slot = st.beam_slot[(e + r) * Kmax + k];
      if (slot >= 0 && slot < S) a.flags[slot] = 1;
    }
  __syncthreads();
  // ---- their numbers: ascending slot index
  int n = 0;
  for (int base = 0; base < S; base += UIS_MIGRATE_THREADS) {
    const int s = base + tid;
    const bool f = s < S && a.flags[s] != 0;
    const unsigned long long ball = __ballot(f);
    const int lane = tid & 63, wave = tid >> 6;
    if (lane == 0) s_wave[wave] = __popcll(ball);
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < UIS_MIGRATE_THREADS / 64; ++w) { before += w < wave ? s_wave[w] : 0; total += s_wave[w]; }
    if (f) {
      const int j = n + before + __popcll(ball & ((1ull << lane) - 1ull));
      a.map[s] = j;
      a.slot_of[j] = s;
    }
    n += total;
    __syncthreads();
  }
  const int lists_n = s_off[live];
  const UisBlobLayout l = uis_blob_layout(B, m.Dp, m.Hp, m.depth, N, live, n, lists_n);
  UisBlobRank* ranks = reinterpret_cast<UisBlobRank*>(a.img + l.ranks);
  int32_t* lists = reinterpret_cast<int32_t*>(a.img + l.lists);
  int32_t* cnt = reinterpret_cast<int32_t*>(a.img + l.cnt);
  if (tid < live) ranks[tid] = UisBlobRank{s_K[tid], st.beam_last[e + tid], st.beam_sum[e + tid], st.beam_score[e + tid]};
  for (int r = 0; r < live; ++r) {
    const int K = s_K[r];
    int32_t* dst = lists + 2 * (size_t)s_off[r];
    for (int k = tid; k < K; k += UIS_MIGRATE_THREADS) {
      const int slot = st.beam_slot[(e + r) * Kmax + k];
      dst[k] = slot >= 0 && slot < S ? a.map[slot] : -1;   // (-1: no valid state has it, and no import takes it)
      dst[K + k] = st.beam_blk[(e + r) * Kmax + k];
    }
  }
  for (int j = tid; j < n; j += UIS_MIGRATE_THREADS) cnt[j] = st.pool_cnt[(size_t)u * S + a.slot_of[j]];
  if (tid == 0) { a.ctl[0] = live; a.ctl[1] = nb; a.ctl[2] = 0; a.ctl[3] = n; a.ctl[4] = lists_n; a.ctl[5] = (int32_t)N; }
}

template <bool IMPORT>
__global__ __launch_bounds__(UIS_MIGRATE_THREADS) void k_migrate_copy(DevModel m, DecodeState st, MigrateArgs a) {
  const int tid = threadIdx.x, u = a.u;
  const int live = IMPORT ? a.live : a.ctl[0];
  if (live == 0) return;
  const int n = IMPORT ? a.n : a.ctl[3], lists_n = IMPORT ? a.lists : a.ctl[4], N = IMPORT ? a.N : a.ctl[5];
  const UisBlobLayout l = uis_blob_layout(st.B, m.Dp, m.Hp, m.depth, N, live, n, lists_n);
  if ((int)blockIdx.x < a.slot_groups) {
    const int mean4 = m.Dp / 4, hid4 = m.depth * m.Hp / 4;
    for (int j = blockIdx.x; j < n; j += a.slot_groups) {
      const size_t slot = (size_t)u * st.S + (IMPORT ? j : a.slot_of[j]);
      f32x4* pm = reinterpret_cast<f32x4*>(st.pool_mean + slot * m.Dp);
      f32x4* ph = reinterpret_cast<f32x4*>(st.pool_hid + slot * m.depth * m.Hp);
      f32x4* bm = reinterpret_cast<f32x4*>(a.img + l.mean) + (size_t)j * mean4;
      f32x4* bh = reinterpret_cast<f32x4*>(a.img + l.hid) + (size_t)j * hid4;
      for (int i = tid; i < mean4; i += UIS_MIGRATE_THREADS) { if (IMPORT) pm[i] = bm[i]; else bm[i] = pm[i]; }
      for (int i = tid; i < hid4; i += UIS_MIGRATE_THREADS) { if (IMPORT) ph[i] = bh[i]; else bh[i] = ph[i]; }
    }
    return;
  }
  const long words = (long)N * st.B;
  const long w0 = (long)((int)blockIdx.x - a.slot_groups) * UIS_MIGRATE_TILE_WORDS;
  if (w0 >= words) return;
  const long count = words - w0 < UIS_MIGRATE_TILE_WORDS ? words - w0 : UIS_MIGRATE_TILE_WORDS;
  uint32_t* bp = st.bp + (size_t)st.tau * st.off[u] * st.B + w0;
  uint32_t* rec = reinterpret_cast<uint32_t*>(a.img + l.records) + w0;
  if (IMPORT) migrate_copy_words(bp, rec, count);
  else migrate_copy_words(rec, bp, count);
}

// what a session of this handle expects of a blob
UisBlobShape migrate_shape(const uis_handle* h) {
  const DevModel& m = h->m;
  return UisBlobShape{(uint32_t)UIS_NUMERICS_VERSION, h->stream_state.B, m.D, m.Dp, h->H_model, m.Hp, m.depth, h->hid_map_seg,
                      h->hid_map_seg_p, h->model_hash};
}

int64_t migrate_bound(const uis_handle* h) {
  const uis_handle::Stream& ss = h->stream_state;
  return uis_blob_bound(ss.B, h->m.Dp, h->m.Hp, h->m.depth, ss.cap, ss.Kmax, ss.S);
}

bool migrate_utt(const uis_handle* h, int32_t utt) {
  return (utt >= 0 && utt < h->stream_state.U) ||
         !fail(UIS_ERR_INVALID_ARG, "utterance " + std::to_string(utt) + " is not in [0, " + std::to_string(h->stream_state.U) + ")");
}

void migrate_trace(const char* call, uis_handle* h, int utt, const UisBlobScalars& sc, int64_t bytes, const CallTimer& timer) {
  const uis_handle::Stream& ss = h->stream_state;
  if (CallTimer::env("UIS_MIGRATE_TRACE"))
    fprintf(stderr, "%s: utterance %d window_frames %d committed %lld live %d slots %d bytes %lld prior_table_entries %lld device_ms %.3f "
            "call_ms %.3f persistent %d resident_launches %lld\n", call, utt, sc.N, (long long)sc.committed, sc.live, sc.n,
            (long long)bytes, (long long)ss.log_len, timer.device_ms(), timer.call_ms(), ss.persist ? 1 : 0, (long long)ss.pm_launches);
}

// the slot groups, then a workgroup per tile of the window's record words
unsigned migrate_grid(const MigrateArgs& a, int64_t window_frames, int B) {
  const int64_t words = window_frames * (int64_t)B;
  return (unsigned)(a.slot_groups + (words + UIS_MIGRATE_TILE_WORDS - 1) / UIS_MIGRATE_TILE_WORDS);
}

}  // namespace

UIS_EXPORT int32_t uis_stream_export_bound(uis_handle* h, int32_t utt, int64_t* bytes_out) {
  if (int rc = begin_call(h, "uis_stream_export_bound", UIS_RULE_STREAM_OTHER)) return rc;
  if (!session_of(h, bytes_out != nullptr, "null handle/bytes_out")) return UIS_ERR_INVALID_ARG;
  if (!migrate_utt(h, utt)) return UIS_ERR_INVALID_ARG;
  *bytes_out = migrate_bound(h);
  return UIS_OK;
}

UIS_EXPORT int32_t uis_stream_export(uis_handle* h, int32_t utt, void* blob, int64_t capacity, int64_t* bytes_out) {
  if (int rc = begin_call(h, "uis_stream_export", UIS_RULE_STREAM_OTHER)) return rc;
  if (!session_of(h, blob && bytes_out, "null handle/blob/bytes_out")) return UIS_ERR_INVALID_ARG;
  if (!migrate_utt(h, utt)) return UIS_ERR_INVALID_ARG;
  uis_handle::Stream& ss = h->stream_state;
  const DevModel& m = h->m;
  CallTimer timer{h};
  // ---- the checks
  const int64_t bound = migrate_bound(h);
  if (capacity < bound)
    return fail(UIS_ERR_INVALID_ARG, "blob: " + std::to_string((long long)bound) + " bytes needed (uis_stream_export_bound)");
  int rc;
  DecodeState stv;
  if ((rc = session_enter(h, &stv))) return rc;
  hipStream_t st = h->stream;
  // ---- scratch: [control words][image] come back in one copy; the slot tables stay on the device
  ScratchPlan plan;
  const size_t o_ctl = plan.take(UIS_MIGRATE_CTL_BYTES), o_img = plan.take((size_t)bound), o_flags = plan.take((size_t)ss.S * 4),
               o_map = plan.take((size_t)ss.S * 4), o_slot = plan.take((size_t)ss.S * 4), land = o_flags - o_ctl;
  char* base;
  if ((rc = session_buffers(h, plan, land, &base))) return rc;
  MigrateArgs a{};
  a.u = utt;
  a.slot_groups = std::min(ss.S, UIS_MIGRATE_SLOT_GROUPS);
  a.ctl = reinterpret_cast<int32_t*>(base + o_ctl);
  a.img = base + o_img;
  a.flags = reinterpret_cast<int32_t*>(base + o_flags);
  a.map = reinterpret_cast<int32_t*>(base + o_map);
  a.slot_of = reinterpret_cast<int32_t*>(base + o_slot);
  // ---- pack, copy
  HIPCHK(timer.begin());
  hipLaunchKernelGGL(k_migrate_pack<false>, dim3(1), dim3(UIS_MIGRATE_THREADS), 0, st, m, stv, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_migrate_copy<false>, dim3(migrate_grid(a, ss.have[utt], ss.B)), dim3(UIS_MIGRATE_THREADS), 0, st, m, stv, a);
  HIPCHK(hipGetLastError());
  HIPCHK(timer.end());
  HIPCHK(hipMemcpyAsync(ss.h_land.p, base + o_ctl, land, hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  // ---- the host's side: nothing of the session changes
  const int32_t* ctl = ss.h_land.as<int32_t>();
  const char* img = ss.h_land.as<char>() + (o_img - o_ctl);
  if (ctl[2])
    return fail(UIS_ERR_CLUSTER_CAP, "utterance " + std::to_string(utt) + " has hit the session's max_clusters = " + std::to_string(ss.Kmax) +
                                         ": there is nothing to move (uis_stream_restart brings the slot back)");
  if (ctl[0] == 0)
    return fail(UIS_ERR_INVALID_ARG, "utterance " + std::to_string(utt) + ": the beam is empty (a non-finite frame?): there is nothing to move "
                                         "(uis_stream_restart brings the slot back)");
  UisBlobHeader hd{};
  hd.magic = UIS_BLOB_MAGIC; hd.format = UIS_BLOB_FORMAT; hd.numerics = UIS_NUMERICS_VERSION; hd.look_ahead = 1;
  hd.B = ss.B; hd.D = m.D; hd.Dp = m.Dp; hd.H = h->H_model;
  hd.Hp = m.Hp; hd.depth = m.depth; hd.hid_seg = h->hid_map_seg; hd.hid_seg_p = h->hid_map_seg_p;
  hd.model_hash = h->model_hash;
  UisBlobScalars sc{};
  sc.committed = ss.committed[utt];
  sc.N = ctl[5]; sc.live = ctl[0]; sc.n = ctl[3]; sc.lists = ctl[4];
  sc.win_score = ss.win_score[utt];
  const UisBlobLayout l = uis_blob_layout(ss.B, m.Dp, m.Hp, m.depth, sc.N, sc.live, sc.n, sc.lists);
  if (l.total > bound) return fail(UIS_ERR_HIP, "uis_stream_export: the utterance's tables describe more than the session can hold");
  char* out = static_cast<char*>(blob);
  memcpy(out, &hd, sizeof(hd));
  memcpy(out + l.scalars, &sc, sizeof(sc));
  memcpy(out + l.ranks, img + l.ranks, (size_t)(l.trailer - l.ranks));
  auto pad = [&](int64_t from, int64_t to) { memset(out + from, 0, (size_t)(to - from)); };
  pad(l.lists + 2 * (int64_t)sc.lists * 4, l.cnt);
  pad(l.cnt + (int64_t)sc.n * 4, l.mean);
  pad(l.records + (int64_t)sc.N * ss.B * 4, l.trailer);
  uis_blob_seal(out, l);
  *bytes_out = l.total;
  migrate_trace("uis_stream_export", h, utt, sc, l.total, timer);
  return UIS_OK;
}

UIS_EXPORT int32_t uis_stream_import(uis_handle* h, int32_t utt, const void* blob, int64_t bytes) {
  if (int rc = begin_call(h, "uis_stream_import", UIS_RULE_STREAM_OTHER)) return rc;
  if (!session_of(h, blob != nullptr, "null handle/blob")) return UIS_ERR_INVALID_ARG;
  if (!migrate_utt(h, utt)) return UIS_ERR_INVALID_ARG;
  uis_handle::Stream& ss = h->stream_state;
  const DevModel& m = h->m;
  CallTimer timer{h};
  // ---- the checks: everything that could steer a device address or a loop bound
  const UisBlobShape expect = migrate_shape(h);
  UisBlobInfo info;
  const char* why = "";
  if (uis_blob_validate(blob, bytes, &expect, &info, &why) != UIS_BLOB_OK)
    return fail(UIS_ERR_INVALID_ARG, std::string("uis_stream_import: ") + why);
  const UisBlobScalars& sc = info.sc;
  if (ss.committed[utt] + ss.have[utt] != 0)  // (prime's rule: an emptied window has received frames all the same)
    return fail(UIS_ERR_INVALID_ARG, "utterance " + std::to_string(utt) + " has already received or been primed with " +
                                         std::to_string((long long)(ss.committed[utt] + ss.have[utt])) + " frames: import needs a slot that has received nothing");
  if (sc.N > ss.cap)
    return fail(UIS_ERR_INVALID_ARG, "the blob's window holds " + std::to_string(sc.N) + " frames, the session's max_frames is " + std::to_string((long long)ss.cap));
  if (info.max_K > ss.Kmax)
    return fail(UIS_ERR_CLUSTER_CAP, "a hypothesis of the blob has " + std::to_string(info.max_K) + " clusters, the session's max_clusters is " +
                                         std::to_string(ss.Kmax));
  if (sc.n > ss.S)
    return fail(UIS_ERR_INVALID_ARG, "the blob names " + std::to_string(sc.n) + " pool slots, the session has " + std::to_string(ss.S) + " per utterance");
  // (uis_stream_speakers: a blob whose block-count words carry tags makes the session a tagged one; a persistent
  // session's pushes could never name them again; the 2^24 bound of a tagged session holds for what arrives, too)
  if (info.max_tag > 0 && (ss.st.flags & UIS_FLAG_PERSISTENT))
    return fail(UIS_ERR_UNSUPPORTED, "a UIS_FLAG_PERSISTENT session takes no known speakers: the blob carries speaker tags (uis_stream_speakers)");
  if (int rct = table_status(CallTables::check_tagged_frames("uis_stream_import", ss.tagged || info.max_tag > 0, utt, sc.committed + sc.N))) return rct;
  int rc;
  if ((rc = session_enter(h, nullptr))) return rc;  // (no window table: the target has received nothing)
  hipStream_t st = h->stream;
  // ---- the prior tables: long enough for whatever the window can hold on top of what the utterance brings
  PriorTableGrowth prior;
  if ((rc = prior.reserve(h, sc.committed + sc.N + ss.cap + 2))) return rc;
  // ---- scratch: the blob as it is; it goes up through the pinned block in one copy
  ScratchPlan plan;
  const size_t o_img = plan.take((size_t)bytes);
  char* base;
  if ((rc = session_buffers(h, plan, (size_t)bytes, &base, {&prior.blk, &prior.den}))) return rc;
  if ((rc = prior.upload(h))) return rc;
  memcpy(ss.h_land.p, blob, (size_t)bytes);
  HIPCHK(hipMemcpyAsync(base + o_img, ss.h_land.p, (size_t)bytes, hipMemcpyHostToDevice, st));
  MigrateArgs a{};
  a.u = utt;
  a.N = sc.N; a.live = sc.live; a.n = sc.n; a.lists = sc.lists;
  a.slot_groups = std::max(1, std::min(sc.n, UIS_MIGRATE_SLOT_GROUPS));
  a.min_turn = ss.min_turn[utt];  // (the run of every rank's last-label word is normalised against the TARGET slot's value)
  a.img = base + o_img;
  // ---- unpack, copy
  HIPCHK(timer.begin());
  hipLaunchKernelGGL(k_migrate_pack<true>, dim3(1), dim3(UIS_MIGRATE_THREADS), 0, st, m, ss.st, a);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(k_migrate_copy<true>, dim3(migrate_grid(a, sc.N, ss.B)), dim3(UIS_MIGRATE_THREADS), 0, st, m, ss.st, a);
  HIPCHK(hipGetLastError());
  HIPCHK(timer.end());
  HIPCHK(hipStreamSynchronize(st));
  // ---- the host's side
  ss.have[utt] = sc.N;
  ss.committed[utt] = sc.committed;
  ss.win_score[utt] = sc.win_score;
  ss.tagged = ss.tagged || info.max_tag > 0;
  prior.swap(h);
  h->nb_valid = false;
  migrate_trace("uis_stream_import", h, utt, sc, bytes, timer);
  return UIS_OK;
}
