// call_tables_main.cpp -- the per-call input tables of uisrnn_amd/csrc/uis_call_tables.h.  Stand-alone: built with the
// host compiler (tests/test_call_tables_host.py builds it plain and with -fsanitize=address,undefined), no HIP, no
// library.
//
//   every cell of the rule table, from all four tables pending: what the call reports, what it has consumed, what is
//   still pending; a refused call has consumed the tables its rule takes; uis_stream_prime's two refusals in both
//   orders of pending; a taken table is gone for the next call;
//   the setters: a bad value keeps the old pending table, NULL and length 0 clear, the bias conversion bit for bit;
//   every count-mismatch message for the lengths 0, n - 1 and n + 1;
//   the 2^24 bound of a tagged session from both sides.
// Exit status 0 iff all of that holds.

#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "uis_call_tables.h"

namespace {

int failures = 0;

void expect(bool ok, const char* what, const std::string& detail = "") {
  if (ok) return;
  ++failures;
  if (failures <= 20) fprintf(stderr, "FAILED: %s (%s)\n", what, detail.c_str());
}

uint64_t bits(double v) {
  uint64_t w;
  memcpy(&w, &v, 8);
  return w;
}

const double kModel3[3] = {-0.25, -1.5, -0.8125};
const double kAlpha = 0.6875;

// all four tables pending, each with contents of its own (the stream tags hold a non-zero one)
void set_all(CallTables& t) {
  const int32_t lim[2] = {3, 0};
  const double bias[3] = {0.25, 0.5, 0.75};
  const uint8_t hint[4] = {0, 1, 0, 2}, tags[5] = {0, 0, 9, 0, 0};
  expect(t.set_limits(lim, 2).code == UIS_OK, "set_limits");
  expect(t.set_bias(bias, 3, kModel3, kAlpha).code == UIS_OK, "set_bias");
  expect(CallTables::set_tags(t.hint, hint, 4).code == UIS_OK, "set_tags(hint)");
  expect(CallTables::set_tags(t.stream_tags, tags, 5).code == UIS_OK, "set_tags(stream_tags)");
}

template <typename T>
void check_cell(const char* who, const char* column, PendingTable<T>& table, TableUse use, size_t words) {
  const std::string at = std::string(who) + "/" + column;
  expect(table.pending_set == (use == LEAVE), "pending iff the rule leaves the table", at);
  expect(table.pending.size() == (use == LEAVE ? words : 0), "the pending words", at);
  if (use == LEAVE) return;  // (the call's copy: whatever an earlier call left, not this call's business)
  expect(table.call_set == (use == TAKE), "the call holds the table iff the rule takes it", at);
  expect(table.call.size() == (use == TAKE ? words : 0), "the call's words", at);
  expect((table.data() != nullptr) == (use == TAKE), "data() is null without a call table", at);
}

struct Named { const char* who; TableRule rule; };
const Named kRules[] = {
    {"uis_decode", UIS_RULE_DECODE},           {"uis_score_labels", UIS_RULE_SCORE},      {"uis_stream_begin", UIS_RULE_STREAM_BEGIN},
    {"uis_stream_push", UIS_RULE_STREAM_PUSH}, {"uis_stream_prime", UIS_RULE_STREAM_PRIME}, {"uis_stream_labels", UIS_RULE_STREAM_OTHER},
};
// the table of DESIGN.md section 28, written out: limits, bias, hint, stream_tags
const TableUse kExpected[6][4] = {
    {TAKE, TAKE, TAKE, LEAVE},    {LEAVE, TAKE, REFUSE, LEAVE},   {TAKE, LEAVE, REFUSE, LEAVE},
    {LEAVE, TAKE, REFUSE, TAKE},  {LEAVE, REFUSE, REFUSE, TAKE},  {LEAVE, LEAVE, REFUSE, LEAVE},
};

void the_rules() {
  for (int i = 0; i < 6; ++i) {
    const Named& r = kRules[i];
    const TableUse* e = kExpected[i];
    expect(r.rule.limits == e[0] && r.rule.bias == e[1] && r.rule.hint == e[2] && r.rule.stream_tags == e[3], "the rule as written out", r.who);
    CallTables t;
    set_all(t);
    const TableStatus s = t.begin(r.who, r.rule);
    // what the call reports: the speaker table's refusal before the bias table's, else nothing
    std::string want;
    if (e[2] == REFUSE) want = std::string(r.who) + " takes no known speakers (uis_frame_speakers): the pending table is dropped";
    else if (e[1] == REFUSE) want = std::string(r.who) + " takes no per-frame transition_bias (uis_frame_bias): the pending table is dropped";
    expect(s.code == (want.empty() ? UIS_OK : UIS_ERR_UNSUPPORTED) && s.msg == want, "what begin reports", r.who + (": " + s.msg));
    // every cell, refused call or not: a refused call has consumed the tables its rule takes
    check_cell(r.who, "limits", t.limits, e[0], 2);
    check_cell(r.who, "bias", t.bias3, e[1], 9);
    check_cell(r.who, "hint", t.hint, e[2], 4);
    check_cell(r.who, "stream_tags", t.stream_tags, e[3], 5);
    if (e[3] == TAKE) expect(t.tagged, "tagged is computed at take", r.who);
    // a taken table is gone for the next call: the same rule again finds nothing, refuses nothing
    const TableStatus again = t.begin(r.who, r.rule);
    expect(again.code == UIS_OK && again.msg.empty(), "nothing pending, nothing refused", r.who);
    if (e[0] == TAKE) expect(!t.limits.call_set && t.limits.data() == nullptr, "limits: whatever an earlier call used is gone", r.who);
    if (e[1] == TAKE) expect(!t.bias3.call_set && t.bias3.data() == nullptr, "bias: whatever an earlier call used is gone", r.who);
    if (e[2] == TAKE) expect(!t.hint.call_set && t.hint.data() == nullptr, "hint: whatever an earlier call used is gone", r.who);
    if (e[3] == TAKE) expect(!t.stream_tags.call_set && t.stream_tags.data() == nullptr && !t.tagged, "stream_tags: whatever an earlier call used is gone", r.who);
  }
}

// uis_stream_prime refuses two tables: either alone is reported, both together report the speaker table's -- in both
// orders of setting -- and both are consumed
void primes_two_refusals() {
  const double bias[1] = {0.5};
  const uint8_t hint[1] = {1};
  const std::string no_hint = "uis_stream_prime takes no known speakers (uis_frame_speakers): the pending table is dropped";
  const std::string no_bias = "uis_stream_prime takes no per-frame transition_bias (uis_frame_bias): the pending table is dropped";
  for (int order = 0; order < 4; ++order) {  // 0: bias then hint, 1: hint then bias, 2: bias alone, 3: hint alone
    CallTables t;
    if (order == 0 || order == 2) t.set_bias(bias, 1, kModel3, kAlpha);
    if (order != 2) CallTables::set_tags(t.hint, hint, 1);
    if (order == 1) t.set_bias(bias, 1, kModel3, kAlpha);
    const TableStatus s = t.begin("uis_stream_prime", UIS_RULE_STREAM_PRIME);
    expect(s.code == UIS_ERR_UNSUPPORTED && s.msg == (order == 2 ? no_bias : no_hint), "prime's refusal", std::to_string(order) + ": " + s.msg);
    expect(!t.bias3.pending_set && !t.hint.pending_set && !t.bias3.call_set && !t.hint.call_set, "both consumed", std::to_string(order));
    expect(t.begin("uis_stream_prime", UIS_RULE_STREAM_PRIME).code == UIS_OK, "the next prime is clean", std::to_string(order));
  }
}

void the_setters() {
  CallTables t;
  set_all(t);
  const CallTables before = t;
  // a bad value keeps the old pending table
  const int32_t bad_lim[3] = {1, 4097, 2}, neg_lim[1] = {-1}, edge_lim[2] = {0, 4096};
  TableStatus s = t.set_limits(bad_lim, 3);
  expect(s.code == UIS_ERR_INVALID_ARG && s.msg == "a limit must be in [0, 4096] (0: no bound)", "a limit above 4096", s.msg);
  expect(t.set_limits(neg_lim, 1).code == UIS_ERR_INVALID_ARG, "a negative limit");
  s = t.set_limits(edge_lim, -1);
  expect(s.code == UIS_ERR_INVALID_ARG && s.msg == "negative n_utt", "negative n_utt", s.msg);
  expect(t.limits.pending == before.limits.pending && t.limits.pending_set, "limits: the old table stays");
  const uint8_t bad_tag[3] = {0, 127, 128};
  for (PendingTable<uint8_t>* table : {&t.hint, &t.stream_tags}) {
    s = CallTables::set_tags(*table, bad_tag, 3);
    expect(s.code == UIS_ERR_INVALID_ARG && s.msg == "the speaker tag at frame 2 is above 127 (0: unknown)", "a tag of 128", s.msg);
    s = CallTables::set_tags(*table, bad_tag, -3);
    expect(s.code == UIS_ERR_INVALID_ARG && s.msg == "negative n_frames", "negative n_frames", s.msg);
    expect(table->pending_set && table->pending == (table == &t.hint ? before.hint : before.stream_tags).pending, "tags: the old table stays");
    expect(CallTables::set_tags(*table, bad_tag, 2).code == UIS_OK && table->pending == std::vector<uint8_t>({0, 127}), "127 is a tag");
  }
  const double bad_bias[4][2] = {{0.5, 1.0000001}, {0.5, -1e-300}, {0.5, std::numeric_limits<double>::infinity()}, {0.5, -0.5}};
  for (const double* b : {bad_bias[0], bad_bias[1], bad_bias[2], bad_bias[3]}) {
    s = t.set_bias(b, 2, kModel3, kAlpha);
    expect(s.code == UIS_ERR_INVALID_ARG && s.msg == "transition_bias at frame 1 is outside [0, 1] (NaN: the model's)", "a bias outside [0, 1]", s.msg);
  }
  s = t.set_bias(bad_bias[0], -2, kModel3, kAlpha);
  expect(s.code == UIS_ERR_INVALID_ARG && s.msg == "negative n_frames", "negative n_frames (bias)", s.msg);
  expect(t.bias3.pending == before.bias3.pending && t.bias3.pending_set, "bias: the old table stays");
  // the accepted edges
  expect(t.set_limits(edge_lim, 2).code == UIS_OK && t.limits.pending == std::vector<int32_t>({0, 4096}), "0 and 4096 are limits");
  expect(t.set_limits(edge_lim, 0).code == UIS_OK && t.limits.pending_set && t.limits.pending.empty(), "an empty limits table is a table");
  // NULL and length 0 clear
  set_all(t);
  const uint8_t tag1[1] = {1};
  const double half[1] = {0.5};
  expect(t.set_limits(nullptr, 2).code == UIS_OK && !t.limits.pending_set && t.limits.pending.empty(), "limits: NULL clears");
  expect(t.set_bias(nullptr, 3, kModel3, kAlpha).code == UIS_OK && !t.bias3.pending_set && t.bias3.pending.empty(), "bias: NULL clears");
  expect(CallTables::set_tags(t.hint, nullptr, 4).code == UIS_OK && !t.hint.pending_set && t.hint.pending.empty(), "hint: NULL clears");
  expect(CallTables::set_tags(t.stream_tags, nullptr, 5).code == UIS_OK && !t.stream_tags.pending_set, "stream_tags: NULL clears");
  set_all(t);
  expect(t.set_bias(half, 0, kModel3, kAlpha).code == UIS_OK && !t.bias3.pending_set && t.bias3.pending.empty(), "bias: length 0 clears");
  expect(CallTables::set_tags(t.hint, tag1, 0).code == UIS_OK && !t.hint.pending_set && t.hint.pending.empty(), "hint: length 0 clears");
  expect(CallTables::set_tags(t.stream_tags, tag1, 0).code == UIS_OK && !t.stream_tags.pending_set, "stream_tags: length 0 clears");
  // (NULL with a negative length clears, too: the pointer is looked at first)
  expect(t.set_bias(nullptr, -1, kModel3, kAlpha).code == UIS_OK && CallTables::set_tags(t.hint, nullptr, -1).code == UIS_OK, "NULL comes first");
  // an all-zero stream table is a table, and not a tagged one
  const uint8_t zeros[3] = {0, 0, 0};
  CallTables::set_tags(t.stream_tags, zeros, 3);
  expect(t.begin("uis_stream_push", UIS_RULE_STREAM_PUSH).code == UIS_OK && t.stream_tags.call_set && !t.tagged, "an all-zero table is not tagged");
}

void the_bias_conversion() {
  CallTables t;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const double bias[5] = {nan, 0.0, 1.0, 0.3, 0.5};
  expect(t.set_bias(bias, 5, kModel3, kAlpha).code == UIS_OK && t.bias3.pending.size() == 15, "five frames, three words each");
  const double* w = t.bias3.pending.data();
  for (int k = 0; k < 3; ++k) expect(bits(w[k]) == bits(kModel3[k]), "NaN: the model's words, bit for bit", std::to_string(k));
  expect(bits(w[3]) == bits(0.0) && w[4] == -inf && w[5] == -inf, "0: stay log(1) = +0, switch and new -inf");
  expect(w[6] == -inf && bits(w[7]) == bits(0.0) && bits(w[8]) == bits(0.0 + kAlpha), "1: stay -inf, switch +0, new l_alpha");
  for (int f = 3; f < 5; ++f) {
    const double b = bias[f], l = std::log(b);
    expect(bits(w[3 * f]) == bits(std::log(1.0 - b)) && bits(w[3 * f + 1]) == bits(l) && bits(w[3 * f + 2]) == bits(l + kAlpha),
           "a mid value: std::log's bits", std::to_string(f));
  }
}

void the_count_checks() {
  const int64_t n = 4;
  const char* scopes[3] = {"decode", "call", "session"};
  for (int64_t len : {(int64_t)0, n - 1, n + 1, n}) {
    CallTables t;
    const std::vector<int32_t> lim((size_t)len + 1, 1);  // (+ 1: data() of an empty vector may be NULL, which clears)
    const std::vector<double> bias((size_t)len + 1, 0.5);
    const std::vector<uint8_t> tags((size_t)len + 1, 1);
    t.set_limits(lim.data(), (int32_t)len);
    // (length 0 clears the per-frame tables: then there is no table and no mismatch)
    t.set_bias(bias.data(), len, kModel3, kAlpha);
    CallTables::set_tags(t.hint, tags.data(), len);
    CallTables::set_tags(t.stream_tags, tags.data(), len);
    t.begin("all", TableRule{TAKE, TAKE, TAKE, TAKE});
    const std::string L = std::to_string(len), N = std::to_string(n);
    for (const char* scope : scopes) {
      const std::string tail = std::string(", this ") + scope + " has " + N;
      const bool off = len != n, frames_off = off && len != 0;
      TableStatus s = t.check_limits(scope, n);
      expect(s.code == (off ? UIS_ERR_INVALID_ARG : UIS_OK) && s.msg == (off ? "uis_decode_limits gave " + L + " limits" + tail + " utterances" : ""),
             "limits count", s.msg);
      s = t.check_bias(scope, n);
      expect(s.code == (frames_off ? UIS_ERR_INVALID_ARG : UIS_OK) && s.msg == (frames_off ? "uis_frame_bias gave " + L + " values" + tail + " frames" : ""),
             "bias count", s.msg);
      s = t.check_hint(scope, n);
      expect(s.code == (frames_off ? UIS_ERR_INVALID_ARG : UIS_OK) && s.msg == (frames_off ? "uis_frame_speakers gave " + L + " tags" + tail + " frames" : ""),
             "hint count", s.msg);
      s = t.check_stream_tags(scope, n);
      expect(s.code == (frames_off ? UIS_ERR_INVALID_ARG : UIS_OK) && s.msg == (frames_off ? "uis_stream_speakers gave " + L + " tags" + tail + " frames" : ""),
             "stream_tags count", s.msg);
    }
    // a call of no frames / no utterances against a table of some
    if (len > 0) {
      expect(t.check_limits("decode", 0).msg == "uis_decode_limits gave " + L + " limits, this decode has 0 utterances", "limits against 0");
      expect(t.check_bias("call", 0).msg == "uis_frame_bias gave " + L + " values, this call has 0 frames", "bias against 0");
      expect(t.check_hint("decode", 0).msg == "uis_frame_speakers gave " + L + " tags, this decode has 0 frames", "hint against 0");
      expect(t.check_stream_tags("call", 0).msg == "uis_stream_speakers gave " + L + " tags, this call has 0 frames", "stream_tags against 0");
    }
  }
  // no table: any count passes
  const CallTables none;
  expect(none.check_limits("decode", 7).code == UIS_OK && none.check_bias("call", 7).code == UIS_OK && none.check_hint("decode", 7).code == UIS_OK &&
             none.check_stream_tags("call", 7).code == UIS_OK, "no table, no mismatch");
}

void the_tagged_bound() {
  const int64_t end = (int64_t)1 << 24;
  expect(UIS_TAGGED_FRAMES_END == end, "the bound is 2^24");
  for (const char* who : {"uis_stream_push", "uis_stream_prime", "uis_stream_import"}) {
    const std::string want = std::string(who) + ": utterance 3 of a session with known speakers would have received 2^24 frames or more "
                                                "(a cluster's tag shares its block-count word)";
    expect(CallTables::check_tagged_frames(who, true, 3, end - 1).code == UIS_OK, "2^24 - 1 received is accepted", who);
    TableStatus s = CallTables::check_tagged_frames(who, true, 3, end);
    expect(s.code == UIS_ERR_UNSUPPORTED && s.msg == want, "2^24 is refused", s.msg);
    expect(CallTables::check_tagged_frames(who, true, 3, end + 1).code == UIS_ERR_UNSUPPORTED, "2^24 + 1 is refused", who);
    expect(CallTables::check_tagged_frames(who, false, 3, end).code == UIS_OK && CallTables::check_tagged_frames(who, false, 3, 0x7fffff00ll).code == UIS_OK,
           "an untagged session has no such bound", who);
  }
  // the push side, as uis_stream_push forms it: `session tagged || the call's table tagged`
  const uint8_t zeros[2] = {0, 0}, tags[2] = {0, 5};
  for (int session_tagged = 0; session_tagged < 2; ++session_tagged)
    for (int call_tagged = 0; call_tagged < 2; ++call_tagged) {
      CallTables t;
      CallTables::set_tags(t.stream_tags, call_tagged ? tags : zeros, 2);
      expect(t.begin("uis_stream_push", UIS_RULE_STREAM_PUSH).code == UIS_OK && t.tagged == (call_tagged != 0), "tagged at take");
      const bool any = session_tagged || call_tagged;
      expect(CallTables::check_tagged_frames("uis_stream_push", session_tagged || t.tagged, 0, end - 1).code == UIS_OK, "2^24 - 1 passes");
      // (an untagged session with an all-zero table takes its 2^24th frame; a tagged session or a tagged call does not)
      expect(CallTables::check_tagged_frames("uis_stream_push", session_tagged || t.tagged, 0, end).code == (any ? UIS_ERR_UNSUPPORTED : UIS_OK),
             "2^24: refused iff the session or the call is tagged", std::to_string(session_tagged) + std::to_string(call_tagged));
    }
}

}  // namespace

int main() {
  the_rules();
  primes_two_refusals();
  the_setters();
  the_bias_conversion();
  the_count_checks();
  the_tagged_bound();
  if (failures) {
    fprintf(stderr, "call_tables: %d check(s) failed\n", failures);
    return 1;
  }
  printf("call_tables: ok\n");
  return 0;
}
