// turn_tables_main.cpp -- the fifth per-call table of csrc/uis_call_tables.h (uis_min_turn's) on the host: what every
// rule does with a pending table, the order of the refusals, the setter's validation and the count check.  Built with
// the host compiler alone by tests/test_turn_host.py; tests/call_tables_main.cpp holds the other four columns.
#include <cstdio>
#include <string>

#include "uis_call_tables.h"

static int failures = 0;
static void expect(bool ok, const char* what) {
  if (!ok) { std::printf("FAILED: %s\n", what); ++failures; }
}

struct Named { const char* who; const TableRule* rule; TableUse want; };

int main() {
  const Named rules[] = {
      {"uis_decode", &UIS_RULE_DECODE, TAKE},           {"uis_score_labels", &UIS_RULE_SCORE, REFUSE},
      {"uis_stream_begin", &UIS_RULE_STREAM_BEGIN, REFUSE}, {"uis_stream_push", &UIS_RULE_STREAM_PUSH, REFUSE},
      {"uis_stream_prime", &UIS_RULE_STREAM_PRIME, REFUSE}, {"uis_stream_labels", &UIS_RULE_STREAM_OTHER, REFUSE}};
  const int32_t three[3] = {0, 3, 32767};
  for (const Named& r : rules) {
    expect(r.rule->min_turn == r.want, r.who);
    CallTables t;
    expect(t.set_min_turn(three, 3).code == UIS_OK, "a valid table is accepted");
    const TableStatus s = t.begin(r.who, *r.rule);
    if (r.want == TAKE) {
      expect(s.code == UIS_OK && t.min_turn.call_set && t.min_turn.data()[1] == 3 && !t.min_turn.pending_set, "taken");
      expect(t.check_min_turn("decode", 3).code == UIS_OK, "the count fits");
      const TableStatus off = t.check_min_turn("decode", 2);
      expect(off.code == UIS_ERR_INVALID_ARG && off.msg == "uis_min_turn gave 3 values, this decode has 2 utterances", "the count message");
    } else {
      expect(s.code == UIS_ERR_UNSUPPORTED &&
                 s.msg == std::string(r.who) + " takes no minimum turn length (uis_min_turn): the pending table is dropped",
             "refused, by name");
      expect(!t.min_turn.call_set && !t.min_turn.pending_set && t.min_turn.data() == nullptr, "the refused table is gone");
    }
    // the table is consumed either way: the same entry point begins again without one
    const TableStatus again = t.begin(r.who, *r.rule);
    expect(again.code == UIS_OK && !t.min_turn.call_set, "nothing is pending for the next call");
  }
  // a rule of four columns (tests/call_tables_main.cpp's rows) leaves the table pending
  {
    CallTables t;
    t.set_min_turn(three, 3);
    const TableRule four{LEAVE, LEAVE, LEAVE, LEAVE};
    expect(t.begin("four columns", four).code == UIS_OK && t.min_turn.pending_set && !t.min_turn.call_set, "left pending");
  }
  // the order of the refusals: known speakers, then the minimum turn length, then the bias
  {
    CallTables t;
    const uint8_t tag[1] = {1};
    const double b[1] = {0.5}, model3[3] = {-1.0, -1.0, -1.0};
    CallTables::set_tags(t.hint, tag, 1);
    t.set_bias(b, 1, model3, 0.0);
    t.set_min_turn(three, 3);
    expect(t.begin("uis_stream_prime", UIS_RULE_STREAM_PRIME).msg.find("(uis_frame_speakers)") != std::string::npos, "speakers first");
    t.set_bias(b, 1, model3, 0.0);
    t.set_min_turn(three, 3);
    expect(t.begin("uis_stream_prime", UIS_RULE_STREAM_PRIME).msg.find("(uis_min_turn)") != std::string::npos, "then the turn length");
    expect(t.begin("uis_stream_prime", UIS_RULE_STREAM_PRIME).code == UIS_OK, "every refused table was consumed");
  }
  // the setter: NULL clears, a bad value or count leaves the pending table as it was
  {
    CallTables t;
    const int32_t low[2] = {3, -1}, high[1] = {32768}, edge[1] = {32767};
    expect(t.set_min_turn(low, 2).code == UIS_ERR_INVALID_ARG && !t.min_turn.pending_set, "-1 is refused");
    expect(t.set_min_turn(high, 1).code == UIS_ERR_INVALID_ARG && !t.min_turn.pending_set, "32768 is refused");
    expect(t.set_min_turn(edge, 1).code == UIS_OK && t.min_turn.pending_set, "32767 is a value");
    expect(t.set_min_turn(low, 2).code == UIS_ERR_INVALID_ARG && t.min_turn.pending.size() == 1, "a bad table leaves the pending one");
    expect(t.set_min_turn(edge, -1).code == UIS_ERR_INVALID_ARG, "a negative count");
    expect(t.set_min_turn(nullptr, 0).code == UIS_OK && !t.min_turn.pending_set, "NULL clears");
    expect(t.check_min_turn("decode", 5).code == UIS_OK, "no table fits every count");
  }
  if (failures) return 1;
  std::printf("turn_tables: ok\n");
  return 0;
}
