"""The minimum-turn-length sweep over tests/instantiation_cases.py: which m a case decodes under, which utterances are
compared, and their references -- shared by tests/test_turn_host.py (the table bites: on the CPU) and
tests/test_gpu_turn.py (the decode, bit for bit), computed once per process.
"""

import copy
import functools

import primed_ref
import turn_ref
from oracle import oracle

M = 3
# Where m = 3 changes no compared utterance of a case as tests/instantiation_cases.py builds it -- its model keeps every
# speaker for three frames or more anyway, or never changes speaker -- the case is decoded from another seed, or under
# m = 5: {Case.name: (seed, m)}, the first pair of seeds 0 .. 8 x m 3, 2, 5 that changes a label, empties no beam and
# keeps the survivors inside the case's cap (found on the CPU).  A case's seed makes its MODEL as well as its
# utterances (instantiation_cases._params), and whatever instantiation_cases._SEEDS chose the original seed for -- three
# clusters in some hypothesis of the decode without a rule -- is not kept: here only the conditions above count, and
# the GPU sweep asserts the instantiation that ran.  m = 2 met the conditions nowhere that m = 3 did not; m = 5 did.
OTHER = {
    'rs-H128-D256-v1/exact': (2, 3), 'resident-H128-D256-v0/exact': (2, 3), 'big-H128-D256-v0/exact': (2, 3),
    'big-H256-D512-v0/padded': (2, 3), 'big-H128-D512-v0/padded': (0, 5), 'big_ws-H128-D256-v0/exact': (2, 3),
    'window-H128-D256-v0/exact': (8, 5), 'window-H128-D256-v0/padded': (0, 5), 'window-H256-D512-v0/padded': (1, 5),
    'deep-H128-D256-v0/exact': (1, 5)}
# ... and no such pair exists for these: they are decoded and compared under m = 3 all the same, and their rows bite
# through their other cases (tests/test_turn_host.py holds every ROW to "some compared utterance changes")
QUIET = ('resident-H256-D512-v0/exact', 'big-H512-D512-v0/seg3', 'big-H256-D512-v0/exact', 'window-H512-D512-v0/seg3',
         'deep-H512-D512-v0/seg3')


def case_of(case):
  """The case as the sweep decodes it: tests/instantiation_cases.py's, from OTHER's seed where it names one."""
  if case.name not in OTHER:
    return case
  other = copy.copy(case)
  other.seed = OTHER[case.name][0]
  return other


def checked_utterances(n_utt):
  """As tests/test_gpu_known.py: every utterance of a row with up to four; of the rows with few every other one and the
  single-frame one; of the many-utterance rows every eighth."""
  if n_utt <= 4:
    return list(range(n_utt))
  if n_utt <= 40:
    return [u for u in range(n_utt) if u % 2 == 0 or u == 1]
  return list(range(0, n_utt, 8))


@functools.lru_cache(maxsize=None)
def case_reference(case, ncl):
  """Of case_of(case): (that case, its utterances, m per utterance, the oracle's decode without a rule, {u:
  turn_ref.decode under m} of the checked utterances)."""
  oracle.lib()
  case = case_of(case)
  seqs = case.utterances(ncl)
  ms = [OTHER.get(case.name, (0, M))[1]] * len(seqs)
  free = oracle.decode(case.params(), seqs, case.beam, case.look_ahead, case.test_iteration, n_threads=8)
  model = primed_ref.Model(case.params())
  ref = {u: turn_ref.decode(model, seqs[u], case.beam, case.look_ahead, case.test_iteration, m=ms[u])
         for u in checked_utterances(len(seqs))}
  return case, seqs, ms, free, ref
