// uis_poison.h -- UIS_POISON_WORKSPACE=<32-bit hex word>: every API call fills the working memory it is about to
// use with that word before its first write (tests/test_gpu_poison.py).  Off by default;
// unset, the knob costs the one getenv of from_env() per call and nothing else.
//
// What is filled is what a call may read without having written it in a correct program only by accident: the
// workspace arena (place_workspace() in uis_workspace.hip fills what it has just placed: the arena, or every buffer
// of workspace_list() and k_decode_rs's stretch), a session's tables (stream_alloc, block by block), the staging
// buffers, the readouts' and the trainer's scratch.  What a call defines as input
// carried over from an earlier call (the last decode's tables for the readouts, `resume` between the launches of a
// split decode, a session's state between pushes, the labels uis_eval_last_decode reads, the trainer's parameters
// and moments) is never filled.
//
// Ordering.  A device fill is enqueued on the stream the caller names, always the stream on which the call's own
// first write is enqueued or which every other stream of the call waits for: uis_decode* fill on the handle's
// stream BEFORE ev_begin is recorded there, and the copy stream (every H2D piece, the scatter), and through ev_pre
// the group streams, wait for ev_begin before they touch anything; the sessions, the readouts, uis_score_labels and
// uis_eval_* run on the handle's stream alone, the trainer on its own.  Every call leaves its streams drained, so a
// fill never overtakes an earlier call's work.  A host fill (pinned blocks) is done by the calling thread before it
// posts the cast team (a mutex hands the block over), before it enqueues the copy that lands in the block, or
// before it initialises the mailbox.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

struct UisPoison {
  bool on = false;
  uint32_t word = 0;
  static UisPoison from_env() {
    UisPoison p;
    if (const char* e = getenv("UIS_POISON_WORKSPACE")) {
      p.on = true;
      p.word = (uint32_t)strtoul(e, nullptr, 16);
    }
    return p;
  }
  // `bytes` of device memory at p (4-byte aligned, as every allocation is), asynchronously on `stream`
  hipError_t device(void* p, size_t bytes, hipStream_t stream) const {
    if (!on || !p || !bytes) return hipSuccess;
    hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(p), (int)word, bytes / 4, stream);
    if (e == hipSuccess && bytes % 4)  // (an allocation's odd tail: the word's low byte)
      e = hipMemsetAsync(static_cast<char*>(p) + (bytes & ~(size_t)3), (int)(word & 0xffu), bytes % 4, stream);
    return e;
  }
  // `bytes` of host memory at p, by the calling thread
  void host(void* p, size_t bytes) const {
    if (!on || !p) return;
    uint32_t* w = static_cast<uint32_t*>(p);
    for (size_t i = 0; i < bytes / 4; ++i) w[i] = word;
    for (size_t i = bytes & ~(size_t)3; i < bytes; ++i) static_cast<unsigned char*>(p)[i] = (unsigned char)(word & 0xffu);
  }
};
