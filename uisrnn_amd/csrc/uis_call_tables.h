// uis_call_tables.h -- the per-call input tables of the C ABI: set by one call (uis_decode_limits, uis_frame_bias,
// uis_frame_speakers, uis_stream_speakers, uis_min_turn), then taken, refused or left pending by the calls that follow.  Plain C++:
// the tables, the rule of every kind of entry point as data, the setters' validation, the count checks and the 2^24
// bound of a tagged session -- no HIP type; tests/call_tables_main.cpp builds it with the host compiler alone.
//
// Which entry point does what (tests/test_gpu_call_tables.py pins it from outside):
//   entry points                                  limits  bias    hint    stream_tags  min_turn
//   uis_decode, uis_decode_f64, uis_decode_device,
//   uis_tensors_decode                            take    take    take    leave        take
//   uis_score_labels, uis_score_speakers,
//   uis_speaker_profiles                          leave   take    refuse  leave        refuse
//   uis_stream_begin                              take    leave   refuse  leave        refuse
//   uis_stream_push, uis_tensors_stream_push      leave   take    refuse  take         refuse
//   uis_stream_prime                              leave   refuse  refuse  take         refuse
//   every other uis_stream_* call                 leave   leave   refuse  leave        refuse
//   everything else (uis_ingest_tensors too)      begins no call: touches nothing
// A new entry point picks a rule; a new table adds a column.
#ifndef UIS_CALL_TABLES_H_
#define UIS_CALL_TABLES_H_

#include <stdint.h>

#include <cmath>
#include <string>
#include <vector>

#include "uisrnn_hip.h"

// a cluster's tag shares its block-count word (uis_kernels.h's UIS_BLK_TAG_SHIFT, restated because this header stands
// alone): under known speakers no count may reach 2^24
#define UIS_TAGGED_FRAMES_END ((int64_t)1 << 24)
// a hypothesis' run shares its last-label word (uis_kernels.h's UIS_LAST_RUN_SHIFT, likewise restated): 15 bits
#define UIS_MIN_TURN_MAX 32767

// what a function of this header reports: UIS_OK, or a status of uisrnn_hip.h and the text for uis_last_error
struct TableStatus {
  int32_t code = UIS_OK;
  std::string msg;
};

// One table: as its setter left it for the next call that consumes it, and as the running call took it (at that call's
// entry: consumed whether the call succeeds or not).
template <typename T>
struct PendingTable {
  std::vector<T> pending, call;
  bool pending_set = false, call_set = false;
  void set(const T* p, size_t n) { pending.assign(p, p + n); pending_set = true; }
  void clear() { pending.clear(); pending_set = false; }
  void take() { call.swap(pending); call_set = pending_set; clear(); }
  bool drop() {  // (a call that cannot honour the table: was there one?)
    take();
    const bool was = call_set;
    call.clear(); call_set = false;
    return was;
  }
  const T* data() const { return call_set ? call.data() : nullptr; }
};

enum TableUse : uint8_t { LEAVE, TAKE, REFUSE };
struct TableRule { TableUse limits, bias, hint, stream_tags, min_turn = LEAVE; };
constexpr TableRule UIS_RULE_DECODE{TAKE, TAKE, TAKE, LEAVE, TAKE};
constexpr TableRule UIS_RULE_SCORE{LEAVE, TAKE, REFUSE, LEAVE, REFUSE};
constexpr TableRule UIS_RULE_STREAM_BEGIN{TAKE, LEAVE, REFUSE, LEAVE, REFUSE};
constexpr TableRule UIS_RULE_STREAM_PUSH{LEAVE, TAKE, REFUSE, TAKE, REFUSE};
constexpr TableRule UIS_RULE_STREAM_PRIME{LEAVE, REFUSE, REFUSE, TAKE, REFUSE};  // (the prefix is scored with the model's transition_bias)
// (known speakers and the minimum turn length belong to the offline decodes: DESIGN.md sections 26 and 29)
constexpr TableRule UIS_RULE_STREAM_OTHER{LEAVE, LEAVE, REFUSE, LEAVE, REFUSE};

struct CallTables {
  PendingTable<int32_t> limits;      // max_speakers, one per utterance (uis_decode_limits; 0: no bound)
  PendingTable<double> bias3;        // per-frame transition_bias as {lp_stay, lp_sw, lp_new} (uis_frame_bias)
  PendingTable<uint8_t> hint;        // known speakers of a decode, one tag per frame (uis_frame_speakers; 0: unknown)
  PendingTable<uint8_t> stream_tags; // known speakers of a push / a prime, in that call's frame order (uis_stream_speakers)
  PendingTable<int32_t> min_turn;    // minimum turn length, one per utterance (uis_min_turn; 0 and 1: no rule)
  bool tagged = false;               // the running call's stream_tags hold a non-zero tag

  // ---- an entry point begins: every table its rule names is consumed first, whichever refusal is then reported (the
  // speaker table's first, then the minimum turn length's, then the bias table's)
  TableStatus begin(const char* who, const TableRule& rule) {
    const bool no_limits = use(limits, rule.limits), no_bias = use(bias3, rule.bias), no_hint = use(hint, rule.hint),
               no_tags = use(stream_tags, rule.stream_tags), no_turn = use(min_turn, rule.min_turn);
    if (rule.stream_tags == TAKE) {
      tagged = false;
      for (uint8_t g : stream_tags.call) tagged = tagged || g != 0;
    }
    if (no_hint) return refusal(who, "known speakers (uis_frame_speakers)");
    if (no_turn) return refusal(who, "minimum turn length (uis_min_turn)");
    if (no_bias) return refusal(who, "per-frame transition_bias (uis_frame_bias)");
    if (no_limits) return refusal(who, "max_speakers (uis_decode_limits)");
    if (no_tags) return refusal(who, "known speakers of a session (uis_stream_speakers)");
    return {};
  }

  // ---- the setters: NULL or length 0 clears; a bad value leaves the pending table as it was
  TableStatus set_limits(const int32_t* v, int32_t n_utt) {
    if (!v) { limits.clear(); return {}; }
    if (n_utt < 0) return {UIS_ERR_INVALID_ARG, "negative n_utt"};
    for (int u = 0; u < n_utt; ++u)
      if (v[u] < 0 || v[u] > 4096) return {UIS_ERR_INVALID_ARG, "a limit must be in [0, 4096] (0: no bound)"};
    limits.set(v, (size_t)n_utt);
    return {};
  }
  TableStatus set_min_turn(const int32_t* v, int32_t n_utt) {
    if (!v) { min_turn.clear(); return {}; }
    if (n_utt < 0) return {UIS_ERR_INVALID_ARG, "negative n_utt"};
    for (int u = 0; u < n_utt; ++u)
      if (v[u] < 0 || v[u] > UIS_MIN_TURN_MAX) return {UIS_ERR_INVALID_ARG, "a minimum turn length must be in [0, 32767] (0 and 1: no rule)"};
    min_turn.set(v, (size_t)n_utt);
    return {};
  }
  // (hint and stream_tags)
  static TableStatus set_tags(PendingTable<uint8_t>& table, const uint8_t* tags, int64_t n_frames) {
    if (!tags || n_frames == 0) { table.clear(); return {}; }
    if (n_frames < 0) return {UIS_ERR_INVALID_ARG, "negative n_frames"};
    for (int64_t t = 0; t < n_frames; ++t)
      if (tags[t] > 127) return {UIS_ERR_INVALID_ARG, "the speaker tag at frame " + std::to_string(t) + " is above 127 (0: unknown)"};
    table.set(tags, (size_t)n_frames);
    return {};
  }
  // model3: the model's own {lp_stay, lp_sw, lp_new} (a NaN entry copies them); l_alpha: log(crp_alpha)
  TableStatus set_bias(const double* bias, int64_t n_frames, const double model3[3], double l_alpha) {
    if (!bias || n_frames == 0) { bias3.clear(); return {}; }
    if (n_frames < 0) return {UIS_ERR_INVALID_ARG, "negative n_frames"};
    for (int64_t t = 0; t < n_frames; ++t)
      if (!(std::isnan(bias[t]) || (bias[t] >= 0.0 && bias[t] <= 1.0)))
        return {UIS_ERR_INVALID_ARG, "transition_bias at frame " + std::to_string(t) + " is outside [0, 1] (NaN: the model's)"};
    std::vector<double>& w = bias3.pending;
    w.resize((size_t)n_frames * 3);
    for (int64_t t = 0; t < n_frames; ++t) {
      const double b = bias[t];
      double* o = w.data() + 3 * t;
      if (std::isnan(b)) { o[0] = model3[0]; o[1] = model3[1]; o[2] = model3[2]; continue; }
      // uis_create's expressions, with the C library's log (log(0) = -inf: a hard constraint, dropped by every select)
      o[0] = std::log(1.0 - b);
      o[1] = std::log(b);
      o[2] = o[1] + l_alpha;
    }
    bias3.pending_set = true;
    return {};
  }

  // ---- the running call's table must cover exactly the call's utterances / frames; scope: "decode", "call", "session"
  TableStatus check_limits(const char* scope, int64_t n) const { return check_count(limits, 1, "uis_decode_limits", "limits", scope, n, "utterances"); }
  TableStatus check_bias(const char* scope, int64_t n) const { return check_count(bias3, 3, "uis_frame_bias", "values", scope, n, "frames"); }
  TableStatus check_hint(const char* scope, int64_t n) const { return check_count(hint, 1, "uis_frame_speakers", "tags", scope, n, "frames"); }
  TableStatus check_min_turn(const char* scope, int64_t n) const { return check_count(min_turn, 1, "uis_min_turn", "values", scope, n, "utterances"); }
  TableStatus check_stream_tags(const char* scope, int64_t n) const { return check_count(stream_tags, 1, "uis_stream_speakers", "tags", scope, n, "frames"); }

  // ---- once a session holds a tag, or the running call brings one, no utterance may have received 2^24 frames or more.
  // Host arithmetic, before any device work.
  static TableStatus check_tagged_frames(const char* who, bool tagged, int utt, int64_t received) {
    if (tagged && received >= UIS_TAGGED_FRAMES_END)
      return {UIS_ERR_UNSUPPORTED, std::string(who) + ": utterance " + std::to_string(utt) + " of a session with known speakers would have "
                                       "received 2^24 frames or more (a cluster's tag shares its block-count word)"};
    return {};
  }

 private:
  template <typename T>
  static bool use(PendingTable<T>& table, TableUse how) {  // true: a pending table was refused
    if (how == TAKE) table.take();
    return how == REFUSE && table.drop();
  }
  static TableStatus refusal(const char* who, const char* what) {
    return {UIS_ERR_UNSUPPORTED, std::string(who) + " takes no " + what + ": the pending table is dropped"};
  }
  // (per: the table's words per utterance / frame)
  template <typename T>
  static TableStatus check_count(const PendingTable<T>& table, size_t per, const char* setter, const char* items, const char* scope,
                                 int64_t want, const char* units) {
    if (!table.call_set || (int64_t)table.call.size() == (int64_t)per * want) return {};
    return {UIS_ERR_INVALID_ARG, std::string(setter) + " gave " + std::to_string(table.call.size() / per) + " " + items + ", this " + scope +
                                     " has " + std::to_string(want) + " " + units};
  }
};

#endif  // UIS_CALL_TABLES_H_
