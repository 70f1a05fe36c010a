"""Host-side mirror of ``uisrnn.UISRNN`` for the decode path.

Same constructor, ``load`` / ``save`` / ``predict`` / ``predict_single`` and
module-level ``parallel_predict`` as the reference (uisrnn/uisrnn.py:80-623),
same argument meaning and the same exceptions; the beam search itself runs in
libuisrnn_hip.so on the MI355X through uisrnn_amd._capi.  There is no CPU
implementation behind this class: without the HIP library and a gfx950 device
``predict`` raises.

``fit`` / ``fit_concatenated`` raise NotImplementedError; ``train`` /
``train_concatenated`` (uisrnn_amd/training.py, libuisrnn_hip.so's uis_train_*)
train on the MI355X with the reference's fit semantics.
"""

import struct
import threading
import zlib

import numpy as np

from uisrnn_amd import _capi
from uisrnn_amd import training
from uisrnn_amd import weights

_DEFAULT_MAX_CLUSTERS = 16


def _check_temperature(temperature):
  """The posterior readouts' temperature as a float: a finite number > 0 (ValueError before any device work)."""
  if isinstance(temperature, bool) or not isinstance(temperature, (int, float, np.integer, np.floating)):
    raise ValueError('temperature must be a finite number > 0.')
  value = float(temperature)
  if not np.isfinite(value) or value <= 0.0:
    raise ValueError('temperature must be a finite number > 0, not {!r}.'.format(temperature))
  return value


_MAX_SPEAKERS_LIMIT = 4096  # (the library's own limit: uis_decode_limits)


def _check_max_speakers(max_speakers, args, n_utt):
  """The max_speakers keyword as the library's table: None (no utterance is bounded) or a list of n_utt ints, 0 = no
  bound.  max_speakers=None falls back to args.max_speakers, the way max_clusters rides on the args object.
  ValueError -- before any device work -- for a bool, a float that is not whole, a negative, a value above 4096 or a
  sequence of the wrong length."""
  if max_speakers is None:
    max_speakers = getattr(args, 'max_speakers', None)
  if max_speakers is None:
    return None

  def one(value):
    if value is None:
      return 0
    if isinstance(value, (bool, np.bool_)) or not isinstance(value, (int, float, np.integer, np.floating)):
      raise ValueError('max_speakers must be None, 0 or an integer in [1, {}], not {!r}.'.format(
          _MAX_SPEAKERS_LIMIT, value))
    if isinstance(value, (float, np.floating)) and (not np.isfinite(value) or value != int(value)):
      raise ValueError('max_speakers must be a whole number, not {!r}.'.format(value))
    if not 0 <= int(value) <= _MAX_SPEAKERS_LIMIT:
      raise ValueError('max_speakers must be in [0, {}], not {!r}.'.format(_MAX_SPEAKERS_LIMIT, value))
    return int(value)

  if isinstance(max_speakers, np.ndarray) and max_speakers.ndim == 0:
    max_speakers = max_speakers.item()   # (a 0-d array is a scalar)
  if isinstance(max_speakers, (list, tuple, np.ndarray)):
    values = [one(v) for v in (max_speakers.tolist() if isinstance(max_speakers, np.ndarray) else max_speakers)]
    if len(values) != int(n_utt):
      raise ValueError('max_speakers has {} entries for {} utterances.'.format(len(values), n_utt))
  else:
    values = [one(max_speakers)] * int(n_utt)
  return values if any(values) else None


_MAX_MIN_TURN = 32767  # (a hypothesis' run is fifteen bits of its last-label word: include/uisrnn_hip.h)


def _slot_rules(who, rules):
  """The per-slot rule keywords of the session entries (online, online_pool, predict_primed), which take them as
  **rules: today min_turn alone.  Returns its value (None: not given); TypeError, in Python's own words, for any other."""
  rules = dict(rules)
  value = rules.pop('min_turn', None)
  for name in rules:
    raise TypeError("{}() got an unexpected keyword argument '{}'".format(who, name))
  return value


def _check_min_turn(min_turn, n_utt):
  """The min_turn keyword as the library's table: None (no utterance has a rule) or a list of n_utt ints, 0 and 1 = no
  rule.  min_turn: None, an integer for every utterance, or a sequence with one integer per utterance.  Raises before
  any device work: ValueError for a bool, a negative value, a value above 32767 or a sequence of the wrong length,
  TypeError for a value that is no integer."""
  if min_turn is None:
    return None

  def one(value):
    if isinstance(value, (bool, np.bool_)):
      raise ValueError('min_turn must be an integer in [0, {}], not a bool.'.format(_MAX_MIN_TURN))
    if not isinstance(value, (int, np.integer)):
      raise TypeError('min_turn must be an integer (a number of frames), not {!r}.'.format(value))
    if not 0 <= int(value) <= _MAX_MIN_TURN:
      raise ValueError('min_turn must be in [0, {}], not {!r}.'.format(_MAX_MIN_TURN, value))
    return int(value)

  if isinstance(min_turn, np.ndarray) and min_turn.ndim == 0:
    min_turn = min_turn.item()   # (a 0-d array is a scalar)
  if isinstance(min_turn, (list, tuple, np.ndarray)):
    values = [one(v) for v in (min_turn.tolist() if isinstance(min_turn, np.ndarray) else min_turn)]
    if len(values) != int(n_utt):
      raise ValueError('min_turn has {} entries for {} utterances.'.format(len(values), n_utt))
  else:
    values = [one(min_turn)] * int(n_utt)
  return values if any(v >= 2 for v in values) else None


_MAX_KNOWN_SPEAKERS = 127   # (a cluster's tag is seven bits of its block-count word: include/uisrnn_hip.h)


def _check_known_speakers(known_speakers, lengths, single=False, tables=None):
  """The known_speakers keyword as the library's table: None (nobody is known) or one uint8 array per utterance of that
  utterance's length, 0 = unknown, 1 .. 127 = the utterance's names in the order they first appear.

  known_speakers: None; one sequence per utterance (None for an utterance without known speakers) whose entries are None
  (unknown) or any hashable value (a speaker's name); with single=True the one sequence itself.  Names are compared as
  dict keys are: 1, 1.0 and True are one speaker, 'a' and b'a' two.  A float NaN equals nothing, itself included, so it
  cannot name anybody and is refused.  Raises before any device work: ValueError for a wrong count or length, for more
  than 127 names in one utterance, for a NaN name and for a bool where a sequence is expected, TypeError for an
  unhashable name.

  tables (a session's pushes): one {name: tag} dict per utterance that the call goes on numbering from and adds its new
  names to -- the caller hands in copies and keeps them only if nothing was raised."""
  if known_speakers is None:
    return None

  def refuse_kind(value, who):
    if isinstance(value, (bool, np.bool_)):
      raise ValueError('known_speakers of {} must be a sequence of names (None: unknown), not a bool.'.format(who))
    if isinstance(value, (str, bytes)) or not isinstance(value, (list, tuple, np.ndarray)):
      raise ValueError('known_speakers of {} must be a sequence of names (None: unknown), not {!r}.'.format(
          who, type(value)))

  def one(value, n, who, tags=None):
    if value is None:
      return np.zeros(n, dtype=np.uint8)
    refuse_kind(value, who)
    names = value.tolist() if isinstance(value, np.ndarray) else list(value)
    if len(names) != n:
      raise ValueError('known_speakers of {} has {} entries for {} frames.'.format(who, len(names), n))
    tags, table = {} if tags is None else tags, np.zeros(n, dtype=np.uint8)
    for t, name in enumerate(names):
      if name is None:
        continue
      if isinstance(name, (float, np.floating)) and name != name:   # pylint: disable=comparison-with-itself
        raise ValueError('known_speakers of {} has NaN as a name at frame {}: NaN equals no other name, not even '
                         'itself (None means unknown).'.format(who, t))
      try:
        tag = tags.get(name)
      except TypeError as err:
        raise TypeError('known_speakers of {} has an unhashable name at frame {}: {!r}.'.format(who, t, name)) from err
      if tag is None:
        if len(tags) == _MAX_KNOWN_SPEAKERS:
          raise ValueError('known_speakers of {} names more than {} speakers.'.format(who, _MAX_KNOWN_SPEAKERS))
        tag = tags[name] = len(tags) + 1
      table[t] = tag
    return table

  if single:
    return [one(known_speakers, lengths[0], 'the sequence')]
  refuse_kind(known_speakers, 'a list of sequences')
  if isinstance(known_speakers, np.ndarray) and known_speakers.dtype != object and known_speakers.ndim == 1:
    raise ValueError('known_speakers for a list of sequences must be one sequence of names per sequence.')
  if len(known_speakers) != len(lengths):
    raise ValueError('known_speakers has {} entries for {} utterances.'.format(len(known_speakers), len(lengths)))
  return [one(v, n, 'utterance {}'.format(u), None if tables is None else tables[u])
          for u, (v, n) in enumerate(zip(known_speakers, lengths))]


def _check_transition_bias(transition_bias, lengths, single=False, offline=True):
  """The transition_bias keyword as the library's table: None (the model's value everywhere) or one float64 array per
  utterance, of that utterance's length (NaN: the model's value at that frame).

  transition_bias: None; a scalar (every frame of every utterance); one array per utterance (None for an utterance
  without values of its own); with `single` (one sequence) also that sequence's one array.  lengths: the utterances'
  frame counts.  offline: the utterances start here -- a first value of 0 ("stay with the previous speaker") leaves no
  hypothesis at all and is refused; a session's chunk may well begin with one.
  ValueError -- before any device work -- for a bool, a wrong count or length, a value outside [0, 1] and +-inf."""
  if transition_bias is None:
    return None
  lengths = [int(n) for n in lengths]

  def refuse_kind(value):
    if isinstance(value, (bool, np.bool_)) or (isinstance(value, np.ndarray) and value.dtype == np.bool_):
      raise ValueError('transition_bias must be numbers in [0, 1] (or NaN for the model\'s value), not a bool.')

  def one(value, n, who):
    if value is None:
      return np.full(n, np.nan, dtype=np.float64)
    refuse_kind(value)
    if isinstance(value, (list, tuple)):
      for v in value:
        refuse_kind(v)
    try:
      arr = np.asarray(value, dtype=np.float64)
    except (TypeError, ValueError) as err:
      raise ValueError('transition_bias of {} is not an array of numbers.'.format(who)) from err
    if arr.ndim != 1 or arr.shape[0] != n:
      raise ValueError('transition_bias of {} has shape {} for {} frames.'.format(who, arr.shape, n))
    return np.ascontiguousarray(arr)

  if isinstance(transition_bias, np.ndarray) and transition_bias.ndim == 0:
    refuse_kind(transition_bias)
    transition_bias = transition_bias.item()   # (a 0-d array is a scalar)
  refuse_kind(transition_bias)
  if isinstance(transition_bias, (int, float, np.integer, np.floating)):
    tables = [np.full(n, float(transition_bias), dtype=np.float64) for n in lengths]
  elif not isinstance(transition_bias, (list, tuple, np.ndarray)):
    raise ValueError('transition_bias must be None, a number or arrays of numbers, not {!r}.'.format(type(transition_bias)))
  elif single and len(lengths) == 1 and not (
      len(transition_bias) == 1 and isinstance(transition_bias[0], (list, tuple, np.ndarray))):
    tables = [one(transition_bias, lengths[0], 'the sequence')]
  else:
    if isinstance(transition_bias, np.ndarray) and transition_bias.dtype != object and transition_bias.ndim == 1:
      raise ValueError('transition_bias for a list of sequences must be a number or one array per sequence.')
    if len(transition_bias) != len(lengths):
      raise ValueError('transition_bias has {} entries for {} utterances.'.format(len(transition_bias), len(lengths)))
    tables = [one(v, n, 'utterance {}'.format(u)) for u, (v, n) in enumerate(zip(transition_bias, lengths))]
  for u, b in enumerate(tables):
    bad = ~np.isnan(b) & ~((b >= 0.0) & (b <= 1.0))
    if bad.any():
      t = int(np.flatnonzero(bad)[0])
      raise ValueError('transition_bias of utterance {} is {!r} at frame {}: a value must be in [0, 1] or NaN.'.format(
          u, float(b[t]), t))
    if offline and b.shape[0] and b[0] == 0.0:
      raise ValueError('transition_bias of utterance {} is 0 at its first frame: there is no previous speaker to stay '
                       'with, no hypothesis could exist.'.format(u))
  return tables


def _initial_cluster_cap(args, limits=None):
  """Device table size (clusters per hypothesis) of the first decode attempt.

  The fast select kernel and the one-launch decode need beam_size * (cap + 1) <= 256
  candidates (include/uisrnn_hip.h).  With the default cap 16 a beam wider than 15 would
  leave that path; real diarization rarely opens more than a handful of clusters, so a wide
  beam starts with the largest cap that still fits (never below 8) and the overflow retry
  below doubles it when an utterance does need more.
  """
  explicit = int(getattr(args, 'max_clusters', 0) or 0)
  if explicit:
    return explicit
  fits = 256 // max(int(args.beam_size), 1) - 1
  if int(args.look_ahead) == 1 and 8 <= fits < _DEFAULT_MAX_CLUSTERS:
    return fits
  # max_speakers: every utterance bounded by at most L, and a beam so wide that the rule above has left the fast
  # select: a cap of L brings it back where beam_size * (L + 1) <= 256.  A hypothesis that may not open cluster L + 1
  # cannot overflow it, and the results are the same bits under any sufficient cap.
  # (look_ahead 1 only: the fast select is that path's; at look_ahead 2 a cap of 4 measured 2.4 % slower than the
  # beam 50 / cap 12 shape class -- profiles/limit_rate.json)
  if int(args.look_ahead) == 1 and limits and all(limits) and fits < 8 and int(args.beam_size) * (max(limits) + 1) <= 256:
    return max(limits)
  return _DEFAULT_MAX_CLUSTERS
_MAX_CLUSTERS_LIMIT = 4096   # (the library's own limit: uis_decode_opts.max_clusters)
_DEFAULT_LEVEL_CAP = 32768   # include/uisrnn_hip.h: uis_decode_opts.level_cap's default ...
_MAX_LEVEL_CAP = 524287      # ... and its maximum


def _more_room(cap):
  """The cluster cap of the next attempt, after a hypothesis has opened more clusters than `cap`: twice the room."""
  if cap * 2 > _MAX_CLUSTERS_LIMIT:
    raise RuntimeError('more than {} clusters per hypothesis'.format(_MAX_CLUSTERS_LIMIT))
  return cap * 2


def _first_appearance(ids):
  """Ids of any hashable kind as int32 labels, renamed by order of first appearance."""
  names = {}
  return np.array([names.setdefault(i, len(names)) for i in ids], dtype=np.int32)


def _sequences_with_ids(test_sequences, cluster_ids, name):
  """One array with its id sequence, or a list of arrays with a list of id sequences (the argument `name`), as
  (single, sequences, id sequences)."""
  if isinstance(test_sequences, np.ndarray):
    return True, [test_sequences], [cluster_ids]
  if not isinstance(test_sequences, list):
    raise TypeError('test_sequences should be either a list or numpy array.')
  if not isinstance(cluster_ids, (list, tuple)) or len(cluster_ids) != len(test_sequences):
    raise ValueError('{} must be a list with one id sequence per test sequence.'.format(name))
  return False, test_sequences, list(cluster_ids)


def _chunk_sizes(chunks):
  """Frames per utterance of a push: of one [U, n, D] array (or device tensor), or of a list with an array (or None)
  per utterance."""
  if not isinstance(chunks, (list, tuple)) and getattr(chunks, 'ndim', 0) == 3:
    return [int(chunks.shape[1])] * len(chunks)
  return [0 if c is None else len(c) for c in chunks]


def _stable_ids(gone, n):
  """The first n non-negative integers that are not in the sorted list `gone`."""
  out, skip, c = [], set(gone), 0
  while len(out) < n:
    if c not in skip:
      out.append(c)
    c += 1
  return out


_STATE_TRAILER = struct.Struct('<4sIqqII')   # magic, version, bytes of the library's blob, frames received, labels, retired ids


def _pack_state_trailer(core, final, gone):
  """What only the Python layer knows of an utterance, behind the library's blob `core`: the committed labels the
  session kept, the retired ids, the total received; a CRC-32 of it all at the end."""
  info = _capi.blob_info(core)
  body = _STATE_TRAILER.pack(b'UISP', 1, len(core), info['committed'] + info['N'], len(final), len(gone))
  body += np.asarray(final, dtype='<i4').tobytes() + np.asarray(gone, dtype='<i4').tobytes()
  return body + struct.pack('<I', zlib.crc32(body))


def _unpack_state(blob):
  """bytes of OnlineSession.export_state -> (the library's blob, committed labels, retired ids); ValueError for
  anything else."""
  try:
    blob = bytes(blob)
    info = _capi.blob_info(blob)
  except (TypeError, ValueError) as err:
    raise ValueError('not an exported utterance state: {}'.format(err)) from None
  n_core = info['bytes']
  if n_core < 0 or len(blob) < n_core + _STATE_TRAILER.size + 4:
    raise ValueError('not an exported utterance state: cut short.')
  magic, version, core_bytes, received, n_final, n_gone = _STATE_TRAILER.unpack_from(blob, n_core)
  end = n_core + _STATE_TRAILER.size + 4 * (n_final + n_gone)
  if magic != b'UISP' or version != 1 or core_bytes != n_core or len(blob) != end + 4:
    raise ValueError('not an exported utterance state: bad trailer.')
  if struct.unpack_from('<I', blob, end)[0] != zlib.crc32(blob[n_core:end]):
    raise ValueError('not an exported utterance state: the trailer\'s checksum does not match.')
  if n_final != info['committed'] or received != info['committed'] + info['N']:
    raise ValueError('not an exported utterance state: the trailer does not belong to the blob.')
  at = n_core + _STATE_TRAILER.size
  final = np.frombuffer(blob, dtype='<i4', count=n_final, offset=at).tolist()
  gone = np.frombuffer(blob, dtype='<i4', count=n_gone, offset=at + 4 * n_final).tolist()
  if any(c < 0 for c in final) or any(c < 0 for c in gone) or gone != sorted(set(gone)):
    raise ValueError('not an exported utterance state: bad ids in the trailer.')
  return blob[:n_core], final, gone


class EmptyBeamError(ValueError, IndexError):
  """Every candidate of some decode step was non-finite: no hypothesis survived.

  The reference fails in the same situation, with an exception that depends on WHERE the beam
  empties: `ValueError: max() arg is an empty sequence` at the next step's
  uisrnn/uisrnn.py:531 if frames remain, `IndexError: list index out of range` at
  uisrnn/uisrnn.py:561 after the last one (recorded in tests/golden/probes.json).  This class
  is both, so a caller's handler for either keeps working.  (With a NaN -- not inf -- score the
  reference can instead keep NaN-scored hypotheses, numpy sorts NaN behind inf; that is not
  reproduced: non-finite candidates are never selected here)
  """


class LookAheadWindowError(_capi.HipLibraryError):
  """look_ahead >= 2: inside a window some utterances had more live assignment prefixes than the
  device can hold (beam_size * clusters ^ (look_ahead - 1) hypotheses per intermediate level); the
  reference has no such bound -- it enumerates them one by one.  Round 5: predict() no longer raises
  this at the default capacity (32768 per level): the affected utterances are decoded again on
  their own with eight times the room, up to 524287 hypotheses per level, and only a window beyond
  THAT -- or beyond the device's memory -- ends here.  Lower look_ahead or beam_size for those
  utterances.

  Attributes:
    utterances: indices (into the list given to predict) of the affected utterances.
    results: the label lists of every OTHER utterance (None at the affected positions) -- they were
      decoded again without the affected ones, so nothing valid is thrown away.
  """
  utterances = ()
  results = None


class UISRNN:
  """Unbounded Interleaved-State RNN -- MI355X decode."""

  def __init__(self, args):
    """Construct from the model namespace (uisrnn/uisrnn.py:83-107).

    Weights are freshly initialised like the reference's; use load() or
    load_params() to install trained ones.
    """
    self.observation_dim = args.observation_dim
    self.params = weights.init_params(
        args.observation_dim, args.rnn_hidden_size, args.rnn_depth,
        sigma2=args.sigma2, transition_bias=args.transition_bias,
        crp_alpha=args.crp_alpha)
    self.estimate_sigma2 = args.sigma2 is None
    self.estimate_transition_bias = args.transition_bias is None
    self.device_index = int(getattr(args, 'device_index', 0))
    self.verbosity = getattr(args, 'verbosity', 3)
    self.rnn_dropout = float(getattr(args, 'rnn_dropout', 0.0) or 0.0)
    self.last_train_losses = None  # extension: one {loss, loss1, loss2, loss3} per iteration of train()
    self._decoder = None
    self._extra_decoders = {}
    self.last_stats = None
    self._single_pass = False
    self._state_lock = threading.Lock()  # last_stats / _single_pass: parallel_predict's workers share the model

  # ---- the attributes callers of the reference read and write
  @property
  def transition_bias(self):
    return self.params['transition_bias']

  @transition_bias.setter
  def transition_bias(self, value):
    self.params['transition_bias'] = value
    self._invalidate()

  @property
  def transition_bias_denominator(self):
    return self.params.get('transition_bias_denominator', 0.0)

  @property
  def crp_alpha(self):
    return self.params['crp_alpha']

  @crp_alpha.setter
  def crp_alpha(self, value):
    self.params['crp_alpha'] = value
    self._invalidate()

  @property
  def sigma2(self):
    return self.params['sigma2']

  @sigma2.setter
  def sigma2(self, value):
    self.params['sigma2'] = np.broadcast_to(
        np.asarray(value, dtype=np.float32), (self.observation_dim,)).copy()
    self._invalidate()

  @property
  def rnn_init_hidden(self):
    depth, hid = self.params['rnn_depth'], self.params['rnn_hidden_size']
    return self.params['rnn_init_hidden'].reshape(depth, 1, hid)

  def _invalidate(self):
    if self._decoder is not None:
      self._decoder.close()
    self._decoder = None
    for dec in self._extra_decoders.values():
      dec.close()
    self._extra_decoders = {}

  def load_params(self, params):
    """Install a parameter dict (uisrnn_amd.weights) wholesale."""
    if params['observation_dim'] != self.observation_dim:
      raise ValueError('parameters do not match args.observation_dim')
    self.params = params
    self._invalidate()

  def load(self, filepath):
    """Load a checkpoint written by the reference's save() (uisrnn.py:149-170)."""
    self.load_params(weights.load_checkpoint(filepath))

  def save(self, filepath):
    """Write the reference's checkpoint format (uisrnn.py:135-147)."""
    weights.save_checkpoint(self.params, filepath)

  def fit(self, *unused_args, **unused_kwargs):
    raise NotImplementedError(
        'Training is outside the scope of uisrnn_amd (decode path only): '
        'train with google/uis-rnn and load() the checkpoint.')

  fit_concatenated = fit

  def _log(self, level, msg):
    if self.verbosity >= level:
      print(msg)

  def train_concatenated(self, train_sequence, train_cluster_id, args):
    """The reference's fit_concatenated (uisrnn/uisrnn.py:172-313), trained on the GPU.

    Same arguments, checks and exceptions.  Draws np.random exactly as the reference does
    (permutations, then one mini-batch per iteration); dropout between GRU layers uses the
    trainer's own random stream (uisrnn_amd/training.py).  On return self.params holds the
    trained weights and last_train_losses one record per iteration.
    """
    params, records = training.train_concatenated(
        self, train_sequence, train_cluster_id, args, self._log)
    params['transition_bias'] = self.params['transition_bias']
    params['transition_bias_denominator'] = self.params.get('transition_bias_denominator', 0.0)
    params['crp_alpha'] = self.params['crp_alpha']
    self.params = params
    self._invalidate()
    self.last_train_losses = records

  def train(self, train_sequences, train_cluster_ids, args):
    """The reference's fit (uisrnn/uisrnn.py:315-386), trained on the GPU.

    train_sequences is a list of [length, D] float arrays with a list of label sequences, or one
    concatenated array with its labels.  Estimates (or updates) transition_bias when the model
    was built with transition_bias None, then concatenates, shuffles and trains.
    """
    if isinstance(train_sequences, np.ndarray):
      if self.estimate_transition_bias:
        self._log(2, 'Warning: transition_bias cannot be correctly estimated from a '
                     'concatenated sequence; train_sequences will be treated as a '
                     'single sequence. This can lead to inaccurate estimation of '
                     'transition_bias. Please, consider estimating transition_bias '
                     'before concatenating the sequences and passing it as argument.')
      train_sequences = [train_sequences]
      train_cluster_ids = [train_cluster_ids]
    elif not isinstance(train_sequences, list):
      raise TypeError('train_sequences must be a list or numpy.ndarray')
    if self.estimate_transition_bias:
      bias, denominator = training.estimate_transition_bias(train_cluster_ids)
      bias, denominator = training.merge_transition_bias(
          self.params['transition_bias'], self.transition_bias_denominator, bias, denominator)
      self.params['transition_bias'] = bias
      self.params['transition_bias_denominator'] = denominator
      self._invalidate()
    sequence, labels = training.concatenate_training_data(
        train_sequences, train_cluster_ids, args.enforce_cluster_id_uniqueness, True)
    self.train_concatenated(sequence, labels, args)

  def _get_decoder(self, device=None):
    if self.params['transition_bias'] is None:
      # the reference fails in np.log(None) (uisrnn.py:416-418)
      raise TypeError('transition_bias is None: fit or load a model first.')
    if device is None or device == self.device_index:
      if self._decoder is None:
        self._decoder = _capi.Decoder(self.params, self.device_index)
      return self._decoder
    if device not in self._extra_decoders:  # one handle per further GPU (parallel_predict)
      self._extra_decoders[device] = _capi.Decoder(self.params, device)
    return self._extra_decoders[device]

  def _check_sequence(self, test_sequence):
    """The reference's argument checks, uisrnn/uisrnn.py:510-521."""
    if (not isinstance(test_sequence, np.ndarray) or
        test_sequence.dtype != float):
      raise TypeError('test_sequence should be a numpy array of float type.')
    if test_sequence.ndim != 2:
      raise ValueError('test_sequence must be 2-dim array.')
    if test_sequence.shape[1] != self.observation_dim:
      raise ValueError('test_sequence does not match the dimension specified '
                       'by args.observation_dim.')

  def _offline_arguments(self, test_sequences, args, max_speakers, transition_bias, known_speakers=None,
                         sequences_first=False, min_turn=None):
    """The offline entry points' arguments, checked: (single, sequences, tables) -- single: one array was given, and the
    caller hands out result 0; tables: _decode_batch's keywords limits, bias, speakers and min_turn.

    The first bad argument is the one reported, and the order is part of the interface: an array's sequence comes
    before its bound (the reference's checks first), a list's bound before its sequences -- except with
    sequences_first, parallel_predict's order.  transition_bias and then known_speakers need the lengths and come after
    them; min_turn is last."""
    single = isinstance(test_sequences, np.ndarray)
    if not single and not isinstance(test_sequences, list):
      raise TypeError('test_sequences should be either a list or numpy array.')
    seqs = [test_sequences] if single else test_sequences
    if not (single or sequences_first):
      limits = _check_max_speakers(max_speakers, args, len(seqs))
    for seq in seqs:
      self._check_sequence(seq)
    if single or sequences_first:
      limits = _check_max_speakers(max_speakers, args, len(seqs))
    bias = _check_transition_bias(transition_bias, [s.shape[0] for s in seqs], single=single)
    speakers = _check_known_speakers(known_speakers, [s.shape[0] for s in seqs], single=single)
    turns = _check_min_turn(min_turn, len(seqs))
    return single, seqs, {'limits': limits, 'bias': bias, 'speakers': speakers, 'min_turn': turns}

  def _predict(self, test_sequences, args, max_speakers, transition_bias, known_speakers=None, min_turn=None, **readout):
    """predict / predict_nbest / predict_posteriors: the checked arguments through _decode_batch, whose `readout`
    keyword (n_best or posterior) selects what an utterance's result is."""
    single, seqs, tables = self._offline_arguments(
        test_sequences, args, max_speakers, transition_bias, known_speakers, min_turn=min_turn)
    if not seqs:
      return []
    results = self._decode_batch(seqs, args, **tables, **readout)
    return results[0] if single else results

  def _decode_batch(self, sequences, args, flags=0, device=None, decoder=None, level_cap=0, n_best=0, posterior=None,
                    limits=None, bias=None, speakers=None, min_turn=None, tensors=False, scores_out=None):
    """Decode a list of validated sequences in one lock-step batch.

    `decoder` (a _capi.Decoder built from self.params) overrides the model's own handle for
    `device`; parallel_predict passes one per worker thread.

    n_best > 0 (predict_nbest): an utterance's result is the pair (labelings, scores) of its final
    beam instead of the label list, read right after the decode call whose labels are accepted for it.
    posterior = a temperature (predict_posteriors): the triple (labels, confidence, change), read likewise.
    limits (_check_max_speakers): None, or one int per sequence (0 = no bound); every regrouping below -- the
    overflow retry's subsets, the halves after UIS_ERR_OOM, the look-ahead retry's groups -- takes its members' entries.
    bias (_check_transition_bias): None, or one float64 array per sequence: the per-frame transition_bias table, which
    follows the same regroupings.
    speakers (_check_known_speakers): None, or one uint8 array per sequence: the known speakers' tags, likewise.
    min_turn (_check_min_turn): None, or one int per sequence (0 and 1 = no rule): the minimum turn lengths, likewise.
    tensors (predict_tensors): the sequences are [N_u, D] device tensors; every decode call is decoder.decode_tensors in
    the place of decode_f64 and an utterance's result is its int32 device tensor, a view of that call's label tensor.
    scores_out: None, or a list with one slot per sequence that receives each utterance's score (a numpy float32).
    """
    decoder = decoder or self._get_decoder(device)
    decode_call = decoder.decode_tensors if tensors else decoder.decode_f64

    def take(members):
      """What one decode call is handed for these sequences: the arrays, and their entries of limits, bias, speakers
      and min_turn as decode_f64's keywords (a table that is None is no keyword at all)."""
      tables = {}
      if limits is not None:
        tables['limits'] = [limits[u] for u in members]
      if bias is not None:
        tables['bias'] = np.concatenate([bias[u] for u in members])
      if speakers is not None:
        tables['speakers'] = np.concatenate([speakers[u] for u in members])
      if min_turn is not None:
        tables['min_turn'] = [min_turn[u] for u in members]
      return [sequences[u] for u in members], tables

    def decode(members, level_cap):
      """The results of sequences[u] for u in members, in that order.  Everything below is numbered inside `members`;
      a LookAheadWindowError that leaves here is too."""
      n_utt = len(members)
      results = [None] * n_utt
      failed, errors = [], []   # the utterances whose look-ahead window fits no capacity, and what said so

      def regroup(part, part_cap):
        """Decode the utterances `part` as a group of their own.  A look-ahead overflow in there is numbered inside
        the group: its utterances join `failed` under their numbers here, the other results are kept."""
        try:
          part_results = decode([members[k] for k in part], part_cap)
        except LookAheadWindowError as inner:
          part_results = inner.results
          failed.extend(part[k] for k in inner.utterances)
          errors.append(inner)
        for u, labels in zip(part, part_results):
          results[u] = labels

      def regrouped():
        with self._state_lock:
          self._single_pass = False  # several decodes: no single resident label buffer
        if failed:
          failed.sort()
          exc = LookAheadWindowError('{} (utterances {})'.format(str(errors[0]).split(' (utterances')[0], failed))
          exc.status, exc.utterances, exc.results = _capi.UIS_ERR_UNSUPPORTED, tuple(failed), results
          raise exc from errors[0]
        return results

      pending = list(range(n_utt))
      first_cap = cap = None
      stats = None
      while pending:
        # the float64 arrays go to the library as they are (uis_decode_f64): it casts to float32
        # once, like torch.from_numpy(seq).float() (uisrnn.py:525), on its own threads while the
        # earlier chunks are already travelling to the device
        sub, tables = take(members if len(pending) == n_utt else [members[u] for u in pending])
        if cap is None:
          first_cap = cap = _initial_cluster_cap(args, tables.get('limits'))
        sub_off = np.zeros(len(pending) + 1, dtype=np.int64)
        sub_off[1:] = np.cumsum([s.shape[0] for s in sub])
        try:
          out = decode_call(sub, args.beam_size, args.look_ahead, args.test_iteration,
                            max_clusters=cap, flags=flags, level_cap=level_cap, **tables)
        except _capi.HipLibraryError as err:
          if err.status == _capi.UIS_ERR_OOM and len(pending) > 1:
            # the decode state of this many utterances does not fit the device (or the pinned staging
            # block the host): the reference's predict takes a list of any size (uisrnn.py:588-589), so
            # the list goes in two halves, one after the other -- alternating members, so that a list
            # dealt longest-first stays even -- and each half may halve again.  (A half whose look-ahead
            # window overflowed still lets the other half decode.)
            regroup(pending[0::2], level_cap)
            regroup(pending[1::2], level_cap)
            return regrouped()
          if err.status != _capi.UIS_ERR_UNSUPPORTED or args.look_ahead < 2:
            raise
          # a look-ahead window of some utterances held more assignment prefixes than a level has
          # room for (bit 1 of their flags).  The flags come from the library, sized by the library:
          # a decode that was refused for its OPTIONS (look_ahead > 1024, beam_size > 32767) never
          # started and leaves no flags behind -- that error goes up as it is.
          flags_now = decoder.last_overflow()
          if flags_now.shape[0] != len(pending):
            raise
          level_full = [u for k, u in enumerate(pending) if flags_now[k] & 2]
          if not level_full:
            raise
          # The others' results are valid but were not handed out: decode them again on their own, at the
          # same capacity.  The affected ones get eight times the room per level (the library's default is
          # 32768 hypotheses per level, its maximum 524287), again and again; what ends the retries is the
          # maximum, or the device's memory (UIS_ERR_OOM for a single utterance).
          rest = [u for u in pending if u not in level_full]
          now_cap = level_cap or _DEFAULT_LEVEL_CAP
          more = min(now_cap * 8, _MAX_LEVEL_CAP)
          if now_cap >= _MAX_LEVEL_CAP:   # (no more room to give)
            failed.extend(level_full)
            errors.append(err)
          if rest:
            regroup(rest, level_cap)
          try:
            if now_cap < _MAX_LEVEL_CAP:
              regroup(level_full, more)
          except _capi.HipLibraryError as inner:
            if inner.status != _capi.UIS_ERR_OOM:
              raise
            # One utterance's window does not fit the device at this capacity (the halving inside that call got down
            # to a single utterance and still met UIS_ERR_OOM).  Which one is not known here: the others of this group
            # would fit -- decode the members one by one and name only those that do not (round 6).
            for u in level_full:
              alone = inner   # (a group of one: that call was this utterance's)
              if len(level_full) > 1:
                try:
                  regroup([u], more)
                  alone = None
                except _capi.HipLibraryError as again:
                  if again.status != _capi.UIS_ERR_OOM:
                    raise
                  alone = again
              if alone is not None:
                failed.append(u)
                errors.append(alone)
          return regrouped()
        if stats is None:
          stats = out['stats']
        still = []
        # (the hypotheses of THIS decode call, before a retry of the flagged utterances replaces its state)
        hyps = decoder.last_nbest(n_best) if n_best else None
        post = decoder.last_posterior(posterior) if posterior is not None else None
        for k, u in enumerate(pending):
          if out['overflow'][k]:
            still.append(u)
          else:
            labels = out['labels'][sub_off[k]:sub_off[k + 1]]
            # (device labels are not read back for this: decode_tensors names the emptied beams by their scores)
            if out['empty'][k] if tensors else (labels.size and labels[0] < 0):
              # every candidate of some step was non-finite (nan/inf in the input or the
              # weights): the reference ends up indexing an empty beam_set
              # (uisrnn/uisrnn.py:561) and raises the same exception type
              raise EmptyBeamError('the beam became empty (max() arg is an empty sequence / list '
                                   'index out of range in the reference): non-finite scores in '
                                   'utterance {}'.format(u))
            results[u] = labels if tensors else labels.tolist()
            if scores_out is not None:
              scores_out[members[u]] = out['scores'][k]
            if hyps is not None and labels.size:
              live = int(hyps['counts'][k])
              results[u] = ([row.tolist() for row in hyps['labels'][k][:live]],
                            [float(x) for x in hyps['scores'][k][:live]])
            elif hyps is not None:  # no frames: the one empty labeling, as predict answers, at score 0
              results[u] = ([[]], [0.0])
            if post is not None:
              results[u] = (results[u], post['confidence'][k], post['change'][k])
        pending = still
        if pending:
          # a surviving hypothesis opened more clusters than the device tables
          # hold: decode those utterances again with twice the room
          cap = _more_room(cap)
      with self._state_lock:  # (parallel_predict: the last worker to finish wins, whole)
        self.last_stats = stats
        self._single_pass = cap == first_cap  # no retry: one decode covered everything
      return results

    # (args.level_cap, like args.max_clusters, is an extension: where the retries of a look-ahead window start)
    return decode(list(range(len(sequences))), level_cap or int(getattr(args, 'level_cap', 0) or 0))

  def predict_and_evaluate(self, test_sequences, test_cluster_ids, args):
    """predict() followed by the demo's accuracy step with the labels kept on the device.

    The reference's demo.py:58-64 calls predict and compute_sequence_match_accuracy per
    utterance on the host.  Here the batch is decoded once and the predicted labels, still in
    HBM, are matched against the ground truth by uis_eval_last_decode (confusion matrix +
    exact assignment per utterance in one launch).  Not part of the reference's API.

    Args:
      test_sequences: list of [N_i, D] float arrays.
      test_cluster_ids: list of lists of ground-truth ids (any hashable, e.g. str).
    Returns:
      (predicted label lists, accuracies) -- accuracies equal
      compute_sequence_match_accuracy(truth, predicted) exactly.

    The device kernel handles label sequences with at most 64 distinct ids each (ids below
    65536 after densification); a batch with a sequence beyond that -- the reference's evals.py
    has no such limit, and the cluster-cap retry lets predictions reach 1024 clusters -- is
    scored by the host function evals.compute_sequence_match_accuracy instead, same values.
    """
    from uisrnn_amd import _capi, evals  # pylint: disable=import-outside-toplevel
    if not isinstance(test_sequences, list) or not isinstance(test_cluster_ids, list):
      raise TypeError('test_sequences and test_cluster_ids must be lists')
    if len(test_sequences) != len(test_cluster_ids):
      raise ValueError('one list of cluster ids per test sequence')
    for seq, ids in zip(test_sequences, test_cluster_ids):
      self._check_sequence(seq)
      if len(ids) != seq.shape[0] or not len(ids):
        raise ValueError('sequence1 and sequence2 must be non-empty and of the same size')
    if not test_sequences:
      return [], []
    decoder = self._get_decoder()
    self._single_pass = False
    predicted = self._decode_batch(test_sequences, args)
    truth = np.concatenate([evals.dense_ids(list(ids)) for ids in test_cluster_ids])
    lens = np.array([s.shape[0] for s in test_sequences], dtype=np.int64)
    try:
      if self._single_pass:  # the labels of that one decode are still resident: no upload
        matched = decoder.eval_last_decode(truth, len(test_sequences))
      else:  # the cluster-cap retry decoded a subset last: hand the labels back
        offsets = np.zeros(len(lens) + 1, dtype=np.int64)
        offsets[1:] = np.cumsum(lens)
        flat = np.concatenate([evals.dense_ids(p) for p in predicted])
        matched = decoder.eval_matched(truth, flat, offsets)
    except _capi.HipLibraryError as err:
      if err.status != _capi.UIS_ERR_UNSUPPORTED:
        raise
      # more than 64 distinct ids in some sequence: the host function has no limit
      return predicted, [evals.compute_sequence_match_accuracy(list(ids), list(p))
                         for ids, p in zip(test_cluster_ids, predicted)]
    return predicted, [float(m) / int(n) for m, n in zip(matched, lens)]

  def predict_single(self, test_sequence, args, max_speakers=None, transition_bias=None, known_speakers=None,
                     min_turn=None):
    """Predict labels for one test sequence (uisrnn/uisrnn.py:479-562).

    Args:
      test_sequence: 2-dim float64 numpy array [N, D].
      args: inference namespace (beam_size, look_ahead, test_iteration).
      max_speakers, transition_bias, known_speakers, min_turn: see predict (extensions).

    Returns:
      list of N ints: the predicted cluster id per frame.

    Raises:
      TypeError: test_sequence is not a float numpy array.
      ValueError: wrong rank or observation dimension.
    """
    self._check_sequence(test_sequence)   # (a list too is refused here, in the reference's words)
    return self._predict(test_sequence, args, max_speakers, transition_bias, known_speakers, min_turn)

  def online(self, num_utterances, args, max_frames, persistent=False, horizon=None, retire_at=None, retire_to=None,
             max_speakers=None, **rules):
    """An OnlineSession (streaming decode; extension, see the class).  horizon: None, or the decision
    horizon in frames of a session that commits by itself when a push does not fit its window.  retire_at: None,
    or the cluster count from which the session retires speakers by itself, down to retire_to (default
    retire_at // 2): see OnlineSession.retire.  max_speakers: None, an int or one entry per utterance: the slots'
    bounds (OnlineSession.set_max_speakers).  min_turn (keyword, among **rules): None, an int or one int per utterance: the slots' minimum turn
    lengths (OnlineSession.set_min_turn)."""
    limits = _check_max_speakers(max_speakers, args, num_utterances)
    turns = _check_min_turn(_slot_rules('online', rules), num_utterances)
    if args.look_ahead != 1:
      raise ValueError('online decoding needs look_ahead 1')
    if self.transition_bias is None:
      raise TypeError('transition_bias is None: the model was never fit or loaded')
    return OnlineSession(self, num_utterances, args, max_frames, persistent, horizon, retire_at, retire_to, limits,
                         turns)

  def online_pool(self, slots, args, max_frames, persistent=False, horizon=None, retire_at=None, retire_to=None,
                  max_speakers=None, **rules):
    """A StreamPool over one OnlineSession of `slots` utterances (extension, see the class): for callers
    whose streams begin and end independently of each other."""
    return StreamPool(self.online(slots, args, max_frames, persistent, horizon, retire_at, retire_to, max_speakers,
                                  **rules))

  def predict(self, test_sequences, args, max_speakers=None, transition_bias=None, known_speakers=None, min_turn=None):
    """Predict labels for one sequence or a list of them (uisrnn.py:564-590).

    A list is decoded as ONE lock-step batch on the GPU (the reference loops
    over it serially); the results are the same as calling predict_single on
    each element.

    max_speakers (extension): None, an int, or a sequence with one entry (an int, 0 or None) per sequence: a
    hypothesis that already holds that many clusters opens no further one; everything else is the unbounded decode's
    (DESIGN.md section 24).  None falls back to getattr(args, 'max_speakers', None).  ValueError for a bool, a float
    that is not whole, a negative, a value above 4096 or a wrong length.

    transition_bias (extension): the probability of a speaker change per frame, in the place of
    the model's scalar -- None, a number (every frame), or one array per sequence of that sequence's length (for a single
    sequence: its one array); NaN means the model's value at that frame.  0 keeps a frame with the previous speaker,
    1 makes it change; constraints that contradict each other (or max_speakers) empty the beam: EmptyBeamError.
    ValueError, before any device work, for a bool, a wrong length or count, a value outside [0, 1], +-inf, or 0 at a
    sequence's first frame.

    known_speakers (extension): who speaks at some frames -- None, or one sequence per sequence
    of that sequence's length (for a single sequence: its one sequence; None for a sequence nobody is known in), whose
    entries are None (unknown) or any hashable value, a speaker's name; at most 127 names per sequence.  Frames with
    equal names get equal labels and frames with different names different labels; an unknown frame may join any
    speaker.  The labels returned stay first-appearance integers.  Names that contradict max_speakers or
    transition_bias empty the beam: EmptyBeamError.  Names are compared as dict keys are (1, 1.0 and True are one
    speaker).  ValueError, before any device work, for a wrong count or length, more than 127 names, a float NaN as a
    name, or a bool in the place of a sequence; TypeError for an unhashable name.

    min_turn (extension): how short a turn can be -- None, an int for every sequence, or one int
    per sequence; 0 and 1 mean no rule.  A hypothesis whose last speaker has held the floor for fewer than min_turn
    frames can only continue that speaker, so every completed turn of the decode has at least min_turn frames.  The
    last turn may be shorter (the sequence ends), and with args.test_iteration >= 2 so may the first turn of the labels
    returned, whose run began in the pass before.  A rule that contradicts known_speakers (two names on the first
    two frames under min_turn 3) empties the beam: EmptyBeamError.  ValueError, before any device work, for a wrong count,
    a negative value, a value above 32767 or a bool; TypeError for a value that is no integer.

    Raises:
      TypeError: test_sequences is neither a list nor a numpy array.
      EmptyBeamError: non-finite scores emptied an utterance's beam (the reference raises
        ValueError / IndexError there; this is both).
      LookAheadWindowError: look_ahead >= 2 only -- some utterances had more live assignment
        prefixes inside a window than the device tables hold (a limit the reference does not
        have); the exception names them and carries the other utterances' results.
    """
    return self._predict(test_sequences, args, max_speakers, transition_bias, known_speakers, min_turn)

  def predict_tensors(self, test_sequences, args, lengths=None, max_speakers=None, transition_bias=None,
                      known_speakers=None, min_turn=None, return_scores=False):
    """predict for embeddings that already live on the model's GPU (extension): no copy to the
    host, no cast there, no copy back.

    Args:
      test_sequences: one [N, D] torch tensor, a list of [N_u, D] tensors, or one [U, T, D] tensor with `lengths`
        (one int per utterance, its frames; None: T) -- on the model's device, of dtype float64, float32, float16 or
        bfloat16, with any row stride (a slice of a padded batch, a [:, :D] view); a non-unit inner stride is made
        contiguous here.  The tensors may have been written on torch's current stream just before: the library orders
        itself behind that stream.
      args, max_speakers, transition_bias, known_speakers, min_turn: as predict.
      return_scores: also return each utterance's score (the best hypothesis' negative log-likelihood).

    Returns:
      int32 device tensors of labels, one per utterance (views of one label tensor unless a retry decoded some
      utterances again); for a single [N, D] tensor its one tensor.  With return_scores: (labels, scores), scores a
      float32 numpy array (for a single tensor: its one number).  Bit for bit what predict returns for
      t.double().cpu().numpy().

    Raises:
      TypeError: something that is no torch tensor, an integer or other unsupported dtype, a CPU tensor.
      ValueError: a tensor on another device, a wrong rank or observation dimension, bad lengths; the table errors of
        predict.  All before the library is called.  EmptyBeamError, LookAheadWindowError: as predict.
    """
    import torch  # pylint: disable=import-outside-toplevel
    dim, device = self.observation_dim, self.device_index
    single = isinstance(test_sequences, torch.Tensor) and test_sequences.ndim == 2
    if isinstance(test_sequences, torch.Tensor):
      if single:
        if lengths is not None:
          raise ValueError('lengths belongs to a [U, T, D] tensor.')
        seqs = [_capi._checked_tensor(test_sequences, 2, dim, device, 'test_sequences')[0]]  # pylint: disable=protected-access
      else:
        table, _ = _capi.tensor_table(test_sequences, dim, lengths, device)
        seqs = [test_sequences[u, :int(n)] for u, n in enumerate(table['rows'])]
    elif isinstance(test_sequences, list):
      if lengths is not None:
        raise ValueError('lengths belongs to a [U, T, D] tensor.')
      seqs = [_capi._checked_tensor(t, 2, dim, device, 'test_sequences[{}]'.format(u))[0]  # pylint: disable=protected-access
              for u, t in enumerate(test_sequences)]
    else:
      raise TypeError('test_sequences should be either a list of torch tensors or a torch tensor.')
    sizes = [int(s.shape[0]) for s in seqs]
    tables = {'limits': _check_max_speakers(max_speakers, args, len(seqs)),
              'bias': _check_transition_bias(transition_bias, sizes, single=single),
              'speakers': _check_known_speakers(known_speakers, sizes, single=single),
              'min_turn': _check_min_turn(min_turn, len(seqs))}
    if not seqs:
      return ([], np.zeros(0, dtype=np.float32)) if return_scores else []
    scores = [None] * len(seqs) if return_scores else None
    results = self._decode_batch(seqs, args, tensors=True, scores_out=scores, **tables)
    if single:
      return (results[0], scores[0]) if return_scores else results[0]
    return (results, np.array(scores, dtype=np.float32)) if return_scores else results

  def predict_nbest(self, test_sequences, args, n_best=None, max_speakers=None, transition_bias=None,
                    known_speakers=None, min_turn=None):
    """predict, returning every hypothesis of the final beam instead of the best one (extension).

    Args:
      test_sequences, args: as predict.
      n_best: the most hypotheses wanted per sequence, in [1, args.beam_size] (default: beam_size).
      max_speakers, transition_bias, known_speakers, min_turn: as predict.
    Returns:
      for an array the pair (labelings, scores): at most n_best label lists -- fewer when the final
      beam holds fewer -- best first, and their scores as floats, ascending; labelings[0] is predict's
      answer.  For a list, a list of such pairs.

    Raises:
      what predict raises; ValueError for n_best outside [1, args.beam_size].
    """
    if n_best is None:
      n_best = args.beam_size
    if isinstance(n_best, bool) or not isinstance(n_best, (int, np.integer)):
      raise ValueError('n_best must be an integer in [1, args.beam_size].')
    if not 1 <= int(n_best) <= int(args.beam_size):
      raise ValueError('n_best must be in [1, args.beam_size = {}].'.format(args.beam_size))
    return self._predict(test_sequences, args, max_speakers, transition_bias, known_speakers, min_turn, n_best=int(n_best))

  def predict_posteriors(self, test_sequences, args, temperature=1.0, max_speakers=None, transition_bias=None,
                         known_speakers=None, min_turn=None):
    """predict, with the beam's per-frame confidence in its answer (extension).

    With w_k = softmax(-score_k / temperature) over the hypotheses of the final beam:
      confidence[t]: the weight of the hypotheses whose label at frame t is the returned one.  Label agreement, not
        permutation invariant: an alternative that opened an extra cluster early disagrees on all later frames.
      change[t]: the weight of the hypotheses with a speaker turn between frames t - 1 and t -- invariant to how a
        hypothesis numbers its speakers.  change[0] is 0: the first frame returned has no predecessor (with
        test_iteration > 1 too: the frames returned are the last replay's).

    Args:
      test_sequences, args: as predict.
      temperature: a finite number > 0.  1 is the model's own posterior; a sharply peaked model (a trained D = 256
        one puts all but 1e-3, usually all but 1e-11, on the best hypothesis) needs a larger one to rank its
        uncertain frames.
      max_speakers, transition_bias, known_speakers, min_turn: as predict.
    Returns:
      for an array the triple (labels, confidence, change): predict's answer and two float32 arrays of its length.
      For a list, a list of such triples.  One decode, with predict's cap and level retries.

    Raises:
      what predict raises; ValueError for a temperature that is not a finite number > 0, before any device work.
    """
    temperature = _check_temperature(temperature)
    return self._predict(test_sequences, args, max_speakers, transition_bias, known_speakers, min_turn,
                         posterior=temperature)

  def predict_primed(self, test_sequences, prefix_cluster_ids, args, max_speakers=None, **rules):
    """predict, with the first frames of every sequence already labeled (extension).

    The decode of sequence u starts from the state the model holds after prefix_cluster_ids[u] along its
    first P_u frames (a session primed with them, OnlineSession.prime) and beam-searches the rest: what
    predict computes when its beam is told the opening instead of searching for it.

    Args:
      test_sequences: a [N, D] float array or a list of them (as predict).
      prefix_cluster_ids: P <= N ids for an array (any hashable kind, renamed by order of first
        appearance; may be empty), or a list of such sequences for a list.
      args: inference namespace; look_ahead and test_iteration must be 1 (online decoding).
      max_speakers: as predict.  A prefix with more clusters than its bound is kept: it opens nothing more.
      min_turn (keyword, among **rules): as predict.  The decode goes on from the run the prefix ends in; turns shorter than min_turn inside a
        given prefix are the caller's and are kept.
    Returns:
      N ints for an array, a list of such lists for a list; the first P_u are the renamed prefix.
    Raises:
      what predict raises; ValueError for look_ahead / test_iteration other than 1, a prefix longer than its
      sequence or a list mismatch; _capi.HipLibraryError (status UIS_ERR_INVALID_ARG) for a prefix whose
      likelihood is not finite.
    """
    single, seqs, ids = _sequences_with_ids(test_sequences, prefix_cluster_ids, 'prefix_cluster_ids')
    if int(args.look_ahead) != 1 or int(args.test_iteration) != 1:
      raise ValueError('predict_primed is online decoding: look_ahead and test_iteration must be 1.')
    limits = _check_max_speakers(max_speakers, args, len(seqs))
    turns = _check_min_turn(_slot_rules('predict_primed', rules), len(seqs))
    for seq in seqs:
      self._check_sequence(seq)
    prefixes = []
    for seq, seq_ids in zip(seqs, ids):
      seq_ids = [] if seq_ids is None else (seq_ids.tolist() if isinstance(seq_ids, np.ndarray) else list(seq_ids))
      if len(seq_ids) > seq.shape[0]:
        raise ValueError('prefix_cluster_ids has {} ids for a sequence of {} frames.'.format(
            len(seq_ids), seq.shape[0]))
      prefixes.append(_first_appearance(seq_ids))
    if not seqs:
      return []
    decoder = self._get_decoder()
    results = [None] * len(seqs)
    pending = list(range(len(seqs)))
    cap = _initial_cluster_cap(args, limits)
    while pending:
      lens = [seqs[u].shape[0] for u in pending]
      bound = {} if limits is None else {'limits': [limits[u] for u in pending]}
      decoder.stream_begin(len(pending), args.beam_size, max(max(lens), 1), max_clusters=cap, **bound)
      try:
        if turns is not None:
          decoder.session_set_min_turn([turns[u] for u in pending])
        try:
          decoder.stream_prime([seqs[u][:len(prefixes[u])] for u in pending], [prefixes[u] for u in pending])
        except _capi.HipLibraryError as err:
          if err.status != _capi.UIS_ERR_CLUSTER_CAP:
            raise
          cap = _more_room(cap)  # a prefix with more clusters than the tables hold: the batch again, twice the room
          continue
        decoder.stream_push([seqs[u][len(prefixes[u]):] if seqs[u].shape[0] > len(prefixes[u]) else None
                             for u in pending])
        per_utt, _, overflow, _ = decoder.stream_labels()
      finally:
        decoder.stream_end()
      still = []
      for k, u in enumerate(pending):
        if overflow[k]:
          still.append(u)
          continue
        if per_utt[k].size and per_utt[k][0] < 0:
          raise EmptyBeamError('the beam became empty (max() arg is an empty sequence / list index out of '
                               'range in the reference): non-finite scores in utterance {}'.format(u))
        results[u] = per_utt[k].tolist()
      pending = still
      if pending:
        cap = _more_room(cap)
    return results[0] if single else results

  def _labeled_sequences(self, test_sequences, test_cluster_ids):
    """The argument checks of score_labels / score_speakers: (single, sequences, int32 labels by first appearance)."""
    single, seqs, ids = _sequences_with_ids(test_sequences, test_cluster_ids, 'test_cluster_ids')
    for seq in seqs:
      self._check_sequence(seq)
    labels = []
    for seq, seq_ids in zip(seqs, ids):
      seq_ids = list(np.asarray(seq_ids).tolist()) if isinstance(seq_ids, np.ndarray) else list(seq_ids)
      if len(seq_ids) != seq.shape[0]:
        raise ValueError('test_cluster_ids has {} ids for a sequence of {} frames.'.format(
            len(seq_ids), seq.shape[0]))
      labels.append(_first_appearance(seq_ids))
    return single, seqs, labels

  def _score_in_halves(self, seqs, labels, bias, call, cut):
    """score_labels / score_speakers: one library call over the packed sequences, or -- when their state does not fit
    the device (UIS_ERR_OOM) -- over halves of them, as _decode_batch: alternating members, each half may halve again.

    call(decoder, members, frames, offsets, flat labels, bias=flat table or None) is the library call for the
    utterances `members`; cut(its result, k, u, rows) is what utterance u, the k-th of them with the frames `rows`,
    gets.  Returns that per utterance."""
    lens = [s.shape[0] for s in seqs]
    decoder = self._get_decoder()
    out = [None] * len(seqs)

    def run(members):
      sub_off = np.zeros(len(members) + 1, dtype=np.int64)
      sub_off[1:] = np.cumsum([lens[u] for u in members])
      frames = np.empty((int(sub_off[-1]), self.observation_dim), dtype=np.float32)
      for u, start in zip(members, sub_off[:-1]):
        frames[start:start + lens[u]] = seqs[u]  # float64 -> float32 (RNE), as predict
      try:
        result = call(decoder, members, frames, sub_off, np.concatenate([labels[u] for u in members]),
                      bias=None if bias is None else np.concatenate([bias[u] for u in members]))
      except _capi.HipLibraryError as err:
        if err.status == _capi.UIS_ERR_OOM and len(members) > 1:
          run(members[0::2])
          run(members[1::2])
          return
        raise
      for k, u in enumerate(members):
        out[u] = cut(result, k, u, slice(sub_off[k], sub_off[k + 1]))

    if seqs:
      run(list(range(len(seqs))))
    return out

  def score_labels(self, test_sequences, test_cluster_ids, per_frame=False, transition_bias=None):
    """The model's negative log-likelihood of given labelings (extension).

    The neg_likelihood predict's beam search minimises (uisrnn.py:388-453), applied along the
    given trace from an empty beam state, test_iteration 1: for labels that predict returns with
    test_iteration 1, the score of that decode, bit for bit.  Ids may be of any hashable kind;
    they are renamed by order of first appearance, so the result does not depend on the names.

    Args:
      test_sequences: a [N, D] float array or a list of them (as predict).
      test_cluster_ids: N ids for an array, or a list of such sequences for a list.
      per_frame: also return each frame's float32 loss (their float32 running sum is the score).
      transition_bias: as predict (a first value of 0 is allowed here: that frame's loss is +inf): the labeling is
        scored under the per-frame priors, so that the labels of a test_iteration-1 decode under the same table score
        that decode's score.
    Returns:
      a float (array) or a list of floats (list); with per_frame, a pair (scores, losses) where
      losses is a float32 array per sequence.
    """
    single, seqs, labels = self._labeled_sequences(test_sequences, test_cluster_ids)
    bias = _check_transition_bias(transition_bias, [s.shape[0] for s in seqs], single=single, offline=False)
    out = self._score_in_halves(
        seqs, labels, bias,
        lambda decoder, members, *packed, bias: decoder.score_labels(*packed, want_frame_losses=True, bias=bias),
        lambda result, k, u, rows: (float(result[0][k]), result[1][rows].copy()))
    out_scores, out_losses = [score for score, _ in out], [losses for _, losses in out]
    if single:
      return (out_scores[0], out_losses[0]) if per_frame else out_scores[0]
    return (out_scores, out_losses) if per_frame else out_scores

  def score_speakers(self, test_sequences, test_cluster_ids, transition_bias=None):
    """Every speaker's loss at every frame along given labelings (extension).

    Row t of a sequence's result is what the model would charge for assigning frame t to each speaker open so far, or
    to a new one, given the labels before t: the row _update_beam_state (uisrnn.py:388-453) computes and the decode
    throws away.  Column k is the k-th speaker by first appearance (ids of any hashable kind, renamed as score_labels
    does); the column one past the speakers opened before t is the new-speaker candidate, later columns are +inf.
    The column of the frame's own label is score_labels' per-frame loss, bit for bit.  speaker_posteriors turns the
    rows into soft assignments.

    Args:
      test_sequences, test_cluster_ids, transition_bias: as score_labels.
    Returns:
      a float32 [N, K + 1] array (array), K the sequence's number of speakers, or a list of them (list).
    """
    single, seqs, labels = self._labeled_sequences(test_sequences, test_cluster_ids)
    widths = [int(l.max()) + 2 if l.size else 1 for l in labels]
    bias = _check_transition_bias(transition_bias, [s.shape[0] for s in seqs], single=single, offline=False)
    out = self._score_in_halves(
        seqs, labels, bias,
        lambda decoder, members, *packed, bias: decoder.score_speakers(
            *packed, max(widths[u] for u in members), bias=bias)[1],
        lambda losses, k, u, rows: losses[rows, :widths[u]].copy())
    return out[0] if single else out

  def speaker_profiles(self, test_sequences, test_cluster_ids, transition_bias=None):
    """Who the speakers of given labelings are (extension; uis_speaker_profiles).

    Per speaker of a sequence: how many frames and turns it has, where it first and last speaks, the model's mean for
    it -- the running mean of linear_mean2 outputs that any later frame of the speaker would be scored against --, the
    sum of its frames, and the per-dimension sum of squared residuals of its frames against the mean each was charged
    against.  The mean is what speaker_distances compares across sequences or with enrolled vectors; the residual sums
    are what sigma2_estimate adds up.

    Args:
      test_sequences, test_cluster_ids, transition_bias: as score_labels (the bias reaches `score` only).
    Returns:
      a SpeakerProfile (array) or a list of them (list).  A labeling that is a list of ids is valid by construction.
    """
    single, seqs, labels = self._labeled_sequences(test_sequences, test_cluster_ids)
    _, _, raw_ids = _sequences_with_ids(test_sequences, test_cluster_ids, 'test_cluster_ids')
    names = [list(dict.fromkeys(i.tolist() if isinstance(i, np.ndarray) else list(i))) for i in raw_ids]
    widths = [max(len(n), 1) for n in names]
    bias = _check_transition_bias(transition_bias, [s.shape[0] for s in seqs], single=single, offline=False)

    def cut(result, k, u, rows):
      del rows
      count = len(names[u])
      stats = result['stats'][k, :count]
      return SpeakerProfile(names[u], stats[:, 0].copy(), stats[:, 1].copy(), stats[:, 2].copy(), stats[:, 3].copy(),
                            result['mean'][k, :count].copy(), result['sum_x'][k, :count].copy(),
                            result['sum_r2'][k, :count].copy(), float(result['scores'][k]))

    out = self._score_in_halves(
        seqs, labels, bias,
        lambda decoder, members, *packed, bias: decoder.speaker_profiles(
            *packed, max(widths[u] for u in members), bias=bias),
        cut)
    return out[0] if single else out

  def sigma2_estimate(self, test_sequences, test_cluster_ids):
    """The closed-form maximum-likelihood sigma2 of labeled sequences under the model's OWN means (extension).

    sigma2[d] = sum over sequences and speakers of sum_r2[d] / total frames, where sum_r2 is speaker_profiles': the
    squared residual of every frame against the mean the model charged it against (the running mean of its speaker
    before the frame; the fresh-cluster mean at a speaker's first frame).  Summed on the host in float64, in list
    order.  No training is involved and nothing of the model changes: whether to use the estimate on a new domain is
    the caller's decision (`model.sigma2 = model.sigma2_estimate(...)`).  (The name `estimate_sigma2` is the
    reference's boolean training flag on this class.)

    Returns:
      float64 [observation_dim]; NaN everywhere when the sequences hold no frame.
    """
    profiles = self.speaker_profiles(test_sequences, test_cluster_ids)
    if isinstance(profiles, SpeakerProfile):
      profiles = [profiles]
    total = np.zeros(self.observation_dim, dtype=np.float64)
    frames = 0
    for profile in profiles:
      for k in range(len(profile.ids)):
        total = total + profile.sum_r2[k].astype(np.float64)
        frames += int(profile.frames[k])
    with np.errstate(invalid='ignore', divide='ignore'):
      return total / np.float64(frames)


class SpeakerProfile(object):
  """The speakers of one labeled sequence (UISRNN.speaker_profiles), K of them, in first-appearance order:
    ids      the caller's ids
    frames   int32 [K] frames per speaker;  blocks  int32 [K] turns (maximal runs) per speaker
    first, last  int32 [K] the speaker's first and last frame
    mean     float32 [K, D] the model's running mean for the speaker after its last frame
    sum_x    float32 [K, D] the float32 sum of its frames, in frame order
    sum_r2   float32 [K, D] the float32 sum of squared residuals against the means its frames were charged against
    centroid float64 [K, D] sum_x / frames
    score    the labeling's negative log-likelihood (score_labels')"""

  __slots__ = ('ids', 'frames', 'blocks', 'first', 'last', 'mean', 'sum_x', 'sum_r2', 'score')

  def __init__(self, ids, frames, blocks, first, last, mean, sum_x, sum_r2, score):
    self.ids, self.frames, self.blocks, self.first, self.last = list(ids), frames, blocks, first, last
    self.mean, self.sum_x, self.sum_r2, self.score = mean, sum_x, sum_r2, score

  @property
  def centroid(self):
    return self.sum_x.astype(np.float64) / np.asarray(self.frames, dtype=np.float64)[:, None]


def speaker_distances(model, a, b):
  """The model's distance between every speaker of `a` and every speaker of `b`: float64 [K_a, K_b] of
  sum_d (mean_a[d] - mean_b[d])^2 / (2 sigma2[d]) -- the weighted MSE the decode itself uses between a frame and a
  speaker's mean, here between two means.  On the host.

  Args:
    model: a UISRNN (its sigma2 weighs the dimensions).
    a, b: SpeakerProfiles, session profiles (dicts with 'mean') or [K, D] arrays -- enrolled vectors, say.
  Which speakers are the same person (a threshold, an assignment) is left to the caller.
  """
  def means(p):
    m = p.mean if isinstance(p, SpeakerProfile) else (p['mean'] if isinstance(p, dict) else p)
    m = np.asarray(m, dtype=np.float64)
    if m.ndim != 2 or m.shape[1] != model.observation_dim:
      raise ValueError('speaker means must be [K, observation_dim] arrays.')
    return m
  ma, mb = means(a), means(b)
  weight = 1.0 / (2.0 * np.asarray(model.sigma2, dtype=np.float64).reshape(-1))
  diff = ma[:, None, :] - mb[None, :, :]
  return (diff * diff * weight).sum(axis=2)


def speaker_posteriors(losses, temperature=1.0):
  """Soft speaker assignments from UISRNN.score_speakers' rows: the row-wise softmax of -losses / temperature.

  Args:
    losses: a [N, W] array of per-speaker losses (+inf: no such speaker at that frame).
    temperature: a finite number > 0, as predict_posteriors.
  Returns:
    float64 [N, W]; rows sum to 1, +inf maps to 0, a row that is all +inf (after an invalid label) to NaN.
  """
  temperature = _check_temperature(temperature)
  z = -np.asarray(losses, dtype=np.float64) / temperature
  if z.ndim != 2:
    raise ValueError('losses must be a [N, W] array.')
  with np.errstate(invalid='ignore', divide='ignore'):
    w = np.exp(z - z.max(axis=1, keepdims=True))
    return w / w.sum(axis=1, keepdims=True)


class OnlineSession:
  """Online (streaming) diarization of a fixed set of utterances.

  Not part of the reference's API -- google/uis-rnn only decodes offline, replaying the
  utterance `test_iteration` times (uisrnn/arguments.py:186-193) -- but the model is an
  online one.  A session keeps the beam on the GPU; frames are pushed as they arrive and
  `labels()` returns the currently best hypothesis for everything received.  Equivalent,
  bit for bit, to `predict` with test_iteration=1, look_ahead=1 on the frames received so
  far, whatever the chunking.

    with model.online(num_utterances=2, args=inference_args, max_frames=10000) as session:
      session.push([chunk_a, None])        # [n, D] float arrays; None = nothing new
      session.push([chunk_a2, chunk_b])
      labels = session.labels()            # list of lists of ints, one per utterance
      hyps = session.nbest(3)              # per utterance (labelings, scores) of the three best hypotheses
      final = session.stable_frames()      # per utterance: labels()[u][:final[u]] can no longer change

  A stream longer than max_frames: commit() hands out the labels that are final and moves the session's
  window of max_frames frames behind them; the session keeps them, and labels() / nbest() / stable_frames()
  go on answering for the whole stream.  With horizon=L given to model.online a push that does not fit
  commits by itself, deciding every frame older than the newest L (max_frames >= L + largest chunk + 1):

    with model.online(1, inference_args, max_frames=64, horizon=32) as session:
      for chunk in microphone:             # for ever
        session.push([chunk])
        final = session.commit()           # optional: the labels that became final, to pass on now

  A stream with more speakers than args.max_clusters: retire() deletes clusters that no live hypothesis can still
  name (speakers last heard before the window), and with retire_at=K given to model.online the session does so by
  itself before a push that could take an utterance past K clusters.  The ids the session hands out never change
  and are never reused: a speaker who returns after retirement is a new id.

  Known speakers: push(..., known_speakers=) names who speaks at some of the chunk's frames -- a
  corrected segment, an enrolled voice, a channel tag -- and the stream decodes as predict(..., known_speakers=) would:

      session.push([chunk], known_speakers=[['ann', None, None, 'bob']])   # one name (or None) per frame
      session.speakers()                   # [{'ann': 0, 'bob': 1}]: the label each name's frames carry

  persistent=True (UIS_FLAG_PERSISTENT): the decode kernel stays on the GPU between pushes and is
  fed through a mailbox in pinned host memory -- the lowest push latency (no launch, no copy
  engine), at the price of occupying the whole device until the session closes or has been idle
  for UIS_PERSIST_IDLE_MS (default 50 ms).  Where the model's shape does not allow it the session
  silently uses ordinary launches.
  """

  _final = None   # per utterance the labels committed so far (a list per utterance once the session is open)
  _gone = None    # per utterance the sorted ids of the retired clusters (None: nothing was ever retired)
  _retire_at = None   # the automatic policy: off
  _retire_to = None
  _bound = None   # per utterance an upper bound of K: K at the last query plus the frames pushed since
  _seen = None    # per utterance {id: stream position of its last committed appearance}
  _names = None   # per utterance {name: tag}: its known speakers, numbered 1 .. 127 by first appearance across pushes

  def __init__(self, model, num_utterances, args, max_frames, persistent=False, horizon=None, retire_at=None,
               retire_to=None, limits=None, min_turn=None):
    if horizon is not None and (isinstance(horizon, bool) or not isinstance(horizon, (int, np.integer)) or horizon < 0):
      raise ValueError('horizon must be None or a non-negative integer.')
    cap = None if args is None else _initial_cluster_cap(args)
    self._set_retire_policy(retire_at, retire_to, cap)
    self._model = model
    self._horizon = None if horizon is None else int(horizon)
    self._max_frames = int(max_frames)
    self._final = [[] for _ in range(int(num_utterances))]   # the committed labels, per utterance
    self._beam_size = int(args.beam_size)
    self._decoder = _capi.Decoder(model.params, model.device_index)  # own handle: one session per handle
    self._bound = [0] * int(num_utterances)
    self._seen = [{} for _ in range(int(num_utterances))]
    self.persistent = False
    bound = {} if limits is None else {'limits': limits}
    if persistent:
      try:
        self._decoder.stream_begin(num_utterances, args.beam_size, max_frames, max_clusters=cap,
                                   flags=_capi.UIS_FLAG_PERSISTENT, **bound)
        self.persistent = True
      except _capi.HipLibraryError as err:
        if err.status != _capi.UIS_ERR_UNSUPPORTED:
          raise
    if not self.persistent:
      self._decoder.stream_begin(num_utterances, args.beam_size, max_frames, max_clusters=cap, **bound)
    self._open = True
    self._num_utterances = int(num_utterances)
    if min_turn is not None:
      self._decoder.session_set_min_turn(min_turn)

  def set_min_turn(self, values):
    """Replace the slots' minimum turn lengths between two pushes (uis_session_min_turn): None,
    an int, or one int per utterance; 0 and 1 mean no rule.  A stream pushed under m is bit for bit
    predict(..., min_turn=m) of everything received.  The values belong to the slots: restart keeps them, an imported
    stream decodes on under its new slot's, snapshots do not carry them.  A slot's value can change only while its
    utterance has received nothing (after the session opens or after restart): otherwise _capi.HipLibraryError (status
    UIS_ERR_INVALID_ARG) and no slot changes.  ValueError / TypeError as predict's min_turn."""
    turns = _check_min_turn(0 if values is None else values, self._num_utterances)
    self._decoder.session_set_min_turn(turns if turns is not None else [0] * self._num_utterances)

  def min_turn(self):
    """The slots' minimum turn lengths: a list with an int per utterance (0 and 1: no rule)."""
    return [int(v) for v in self._decoder.session_min_turn()]

  def turns(self):
    """The turn each utterance's best hypothesis is in (uis_session_turns): per utterance (speaker id, run, held) -- the
    id labels() gives the newest frame, for how many frames it has held the floor (saturating at the slot's min_turn; 0
    where the slot has no rule), and whether the rule holds the speaker at the next frame (run < min_turn).
    (-1, 0, False) for an utterance without a live hypothesis or without frames."""
    table = self._decoder.session_turns()
    values = self._decoder.session_min_turn()
    out = []
    for u in range(self._num_utterances):
      label, run = int(table[u, 0]), int(table[u, 1])
      m = int(values[u])
      out.append((self._ids(u, [label])[0], run, bool(label >= 0 and m >= 2 and run < m)))
    return out

  def set_max_speakers(self, values):
    """Replace the slots' bounds between two pushes (uis_stream_limits): None, an int, or one entry (an int, 0 or
    None) per utterance.  A hypothesis that holds at least its utterance's bound opens no further cluster; one
    already above a lowered bound is kept.  The bounds belong to the slots: restart keeps them, an imported stream
    decodes on under its new slot's, snapshots do not carry them.  ValueError as predict's max_speakers."""
    limits = _check_max_speakers(0 if values is None else values, None, self._num_utterances)
    self._decoder.stream_set_limits(limits if limits is not None else [0] * self._num_utterances)

  def max_speakers(self):
    """The slots' bounds: a list with an int or None (no bound) per utterance."""
    return [int(v) if v else None for v in self._decoder.stream_limits()]

  def _name_tables(self):
    if self._names is None:
      self._names = [{} for _ in range(self._num_utterances)]
    return self._names

  def _speaker_tags(self, sizes, known_speakers):
    """A call's known_speakers as (the library's flat uint8 table in the call's frame order, the utterances' name tables
    with the call's new names added) -- (None, None) without the keyword.  Nothing of the session changes here: the
    caller keeps the tables once every check of the call has passed."""
    if known_speakers is None:
      return None, None
    if isinstance(known_speakers, np.ndarray) and known_speakers.ndim == 2:
      known_speakers = list(known_speakers)   # ([U, n] beside [U, n, D]: one row per utterance)
    tables = [dict(t) for t in self._name_tables()]
    per_utt = _check_known_speakers(known_speakers, sizes, tables=tables)
    flat = np.concatenate(per_utt) if per_utt else np.zeros(0, dtype=np.uint8)
    return (flat if flat.size else None), tables

  def speaker_names(self, utterance):
    """The known speakers of an utterance in tag order: names[g - 1] is the name with tag g."""
    names = self._name_tables()[self._utterance(utterance)]
    return sorted(names, key=names.get)

  def speakers(self):
    """Who is who right now (uis_stream_bindings): per utterance {name: label} for the known
    speakers the best hypothesis has bound -- the label labels() gives that speaker's frames.  A name that no frame has
    carried yet, or whose utterance has no live hypothesis, is absent."""
    table = self._decoder.stream_bindings()
    out = []
    for u, names in enumerate(self._name_tables()):
      bound = [(name, int(table[u, tag])) for name, tag in names.items() if table[u, tag] >= 0]
      ids = self._ids(u, [c for _, c in bound])
      out.append({name: ids[i] for i, (name, _) in enumerate(bound)})
    return out

  def profiles(self):
    """Who the speakers of each utterance's best hypothesis are right now (uis_session_profiles):
    per utterance a dict(ids, frames, blocks, names, mean) -- ids: the speakers' ids as labels() gives them (retired ids
    stay gone, handed-out ids never change); frames / blocks: int32 [K], the frames and turns each has over the whole
    stream; names: the known speaker bound to each, or None; mean: float32 [K, D], the model's running mean for each --
    or None for an utterance without a live hypothesis.  Nothing of the session changes."""
    table = self._decoder.stream_profiles()
    out = []
    for u in range(self._num_utterances):
      count = int(table['n_clusters'][u])
      if count < 0:
        out.append(None)
        continue
      stats = table['stats'][u, :count]
      by_tag = {tag: name for name, tag in self._name_tables()[u].items()}
      out.append({'ids': self._ids(u, list(range(count))), 'frames': stats[:, 0].copy(), 'blocks': stats[:, 1].copy(),
                  'names': [by_tag.get(int(tag)) if tag > 0 else None for tag in stats[:, 2]],
                  'mean': table['mean'][u, :count].copy()})
    return out

  def prime(self, chunks, cluster_ids, known_speakers=None):
    """Start utterances from a labeled prefix (uis_stream_prime; extension).

    The session is afterwards in the state it would hold had it received the prefix frames with its beam
    holding only the given labeling: labels() returns the prefix followed by what is decoded, scores are the
    prefix's negative log-likelihood plus the continuation, stable_frames() is at least the prefix length,
    and the prefix frames count against max_frames.

    Args:
      chunks: a list with one [P_u, D] float64 array or None per utterance: the prefix frames.
      cluster_ids: a list with one sequence of P_u ids (any hashable kind; renamed by order of first
        appearance, as score_labels does) or None per utterance.
      known_speakers: None, or as push's: who speaks at the prefix frames.  The primed hypothesis binds each name to
        the cluster its frames are labeled with; within one prefix a name must stay on one id and an id under one name
        (HipLibraryError, UIS_ERR_INVALID_ARG, otherwise).
    Returns:
      a list with the prefix's negative log-likelihood (float) per utterance, None where nothing was primed.
    Raises:
      TypeError / ValueError: a chunk that predict would refuse, in predict's words.
      ValueError: a length mismatch, or an utterance that has already received or been primed with frames.
      _capi.HipLibraryError: the library's refusals (status UIS_ERR_CLUSTER_CAP: a prefix with more clusters
        than the session's max_clusters; UIS_ERR_INVALID_ARG: a prefix longer than max_frames or one whose
        likelihood is not finite).  The session is then as it was.
    """
    n_utt = self._num_utterances
    if not isinstance(chunks, (list, tuple)) or not isinstance(cluster_ids, (list, tuple)):
      raise TypeError('chunks and cluster_ids must be lists with one entry (or None) per utterance.')
    if len(chunks) != n_utt or len(cluster_ids) != n_utt:
      raise ValueError('one chunk and one id sequence (or None) per utterance ({} utterances).'.format(n_utt))
    labels, frames = [None] * n_utt, [None] * n_utt
    received = self._decoder.stream_received()
    if self._final is not None:   # (committed frames have been received all the same, whatever the window holds)
      received = received + np.array([len(f) for f in self._final], dtype=np.int64)
    for u, (chunk, ids) in enumerate(zip(chunks, cluster_ids)):
      if isinstance(ids, np.ndarray):
        ids = ids.tolist()
      n_ids = 0 if ids is None else len(ids)
      if chunk is None:
        if n_ids:
          raise ValueError('utterance {}: {} cluster ids but no frames.'.format(u, n_ids))
        continue
      self._model._check_sequence(chunk)  # pylint: disable=protected-access
      if chunk.shape[0] != n_ids:
        raise ValueError('utterance {}: cluster_ids has {} ids for a prefix of {} frames.'.format(
            u, n_ids, chunk.shape[0]))
      if not n_ids:
        continue
      if received[u]:
        raise ValueError('utterance {} has already received {} frames: a prefix goes in front of '
                         'everything.'.format(u, int(received[u])))
      labels[u] = _first_appearance(ids)
      frames[u] = chunk
    speakers, names = self._speaker_tags([0 if f is None else len(f) for f in frames], known_speakers)
    extra = {} if speakers is None else {'speakers': speakers}
    if names is not None:
      self._names = names
    scores = self._decoder.stream_prime(frames, labels, **extra)
    if self._bound is not None:
      for u in range(n_utt):   # (a prefix of P frames has at most P clusters)
        self._bound[u] += 0 if labels[u] is None else len(labels[u])
    return [float(scores[u]) if labels[u] is not None else None for u in range(n_utt)]

  def _push_bias(self, chunks, transition_bias):
    """push's transition_bias as the library's flat table: the chunk's frames, utterance by utterance."""
    if transition_bias is None:
      return None
    if (not isinstance(chunks, (list, tuple)) and getattr(chunks, 'ndim', 0) == 3 and
        isinstance(transition_bias, np.ndarray) and transition_bias.ndim == 2):
      transition_bias = list(transition_bias)   # ([U, n] beside [U, n, D]: one row per utterance)
    tables = _check_transition_bias(transition_bias, _chunk_sizes(chunks), offline=False)
    return np.concatenate(tables) if tables else np.zeros(0, dtype=np.float64)

  def push(self, chunks, transition_bias=None, known_speakers=None):
    """chunks: a list with one [n, D] float64 array (or None) per utterance, or one [U, n, D]
    float64 array when every utterance received the same number of frames.

    known_speakers: who speaks at some of this push's frames, in the chunk's own layout -- None,
    or one sequence (or None) per utterance of its chunk's length whose entries are None (unknown) or any hashable name.
    The session numbers an utterance's names 1 .. 127 by first appearance across its pushes (restart clears them); the
    128th name is a ValueError before any device work, the other errors are predict's.  The stream is bit for bit
    predict(..., known_speakers=) of everything received.  A persistent session refuses a table like a bias table.

    transition_bias: this push's per-frame probability of a speaker change, in the chunk's own
    layout -- None, a number, one array (or None) per utterance of its chunk's length, or a [U, n] array beside a
    [U, n, D] chunk; NaN = the model's value.  A push without it decodes with the model's value, whatever the last one
    used.  ValueError as predict's; a persistent session refuses a table (HipLibraryError, UIS_ERR_UNSUPPORTED) and
    stays usable."""
    bias = self._push_bias(chunks, transition_bias)
    if bias is not None and not bias.size:
      bias = None
    extra = {} if bias is None else {'bias': bias}
    speakers, names = self._speaker_tags(_chunk_sizes(chunks), known_speakers)
    if speakers is not None:
      extra['speakers'] = speakers
    if names is not None:
      self._names = names
    if self._retire_at is not None:
      self._keep_under_cap(chunks)
    if self._horizon is not None:
      self._make_room(chunks)
    if isinstance(chunks, np.ndarray) and chunks.ndim == 3:
      if chunks.dtype != float:
        raise TypeError('test_sequence should be a numpy array of float type.')
    else:
      # (round 6: one pass over the dtypes -- the reference's TypeError for anything but float64, uisrnn.py:511-513 --
      # the shapes are checked by the one concatenate in _capi.stream_push; the full per-chunk check of the
      # reference's messages only when something is off)
      try:
        plain = {c.dtype for c in chunks} == {np.dtype(float)}
      except AttributeError:
        plain = False
      if not plain:
        for chunk in chunks:
          if chunk is not None and len(chunk):
            self._model._check_sequence(np.asarray(chunk))
      try:
        self._decoder.stream_push(chunks, **extra)
      except ValueError:
        for chunk in chunks:   # (which chunk, in the reference's words)
          if chunk is not None and len(chunk):
            self._model._check_sequence(np.asarray(chunk))
        raise
      return
    self._decoder.stream_push(chunks, **extra)

  def push_tensors(self, chunks, transition_bias=None, known_speakers=None):
    """push for frames that already live on the model's GPU: a list with one [n, D] torch tensor
    (or None) per utterance, or one [U, n, D] tensor -- float64, float32, float16 or bfloat16, any row stride.  The
    frames never leave the device; room-making, the retire policy, transition_bias and known_speakers work as in push,
    and the stream is bit for bit the one push gives for the same values.  A persistent session takes its frames
    through the host: ValueError at once, the session untouched.  TypeError / ValueError as predict_tensors, before the
    library is called."""
    if self.persistent:
      raise ValueError('a persistent session takes no device tensors (its frames travel through the host mailbox): use '
                       'push, or open the session with persistent=False.')
    if len(chunks) != self._num_utterances:
      raise ValueError('one chunk (or None) per utterance')
    # (the checks of every tensor, before any table is built or any room is made)
    table = _capi.tensor_table(chunks, self._model.observation_dim, None, self._model.device_index, 'chunks')
    bias = self._push_bias(chunks, transition_bias)
    extra = {} if bias is None or not bias.size else {'bias': bias}
    speakers, names = self._speaker_tags(_chunk_sizes(chunks), known_speakers)
    if speakers is not None:
      extra['speakers'] = speakers
    if names is not None:
      self._names = names
    if self._retire_at is not None:
      self._keep_under_cap(chunks)
    if self._horizon is not None:
      self._make_room(chunks)
    self._decoder.stream_push_tensors(chunks, table=table, **extra)

  def _make_room(self, chunks):
    """horizon given: a push whose chunk does not fit the window commits first."""
    sizes = np.array(_chunk_sizes(chunks), dtype=np.int64)
    if len(sizes) != self._num_utterances:
      return   # (stream_push refuses it in its own words)
    if ((self._decoder.stream_received() + sizes) <= self._max_frames).all():
      return
    self.commit(self._horizon)
    if ((self._decoder.stream_received() + sizes) > self._max_frames).any():
      raise ValueError('a chunk of {} frames does not fit the session\'s window after a commit: max_frames ({}) must be '
                       'at least horizon + chunk + 1 = {}.'.format(int(sizes.max()), self._max_frames,
                                                                   self._horizon + int(sizes.max()) + 1))

  def commit(self, horizon=None):
    """Hand out the labels that are final and give their room back to the session (uis_stream_commit).

    Without a horizon the stable prefix (stable_frames()) is committed, rounded down to an even count: the
    session's results do not change, only its window moves.  With horizon=L frames older than the newest L are
    decided in favour of the currently best hypothesis as well, and the hypotheses that disagree with it there
    leave the beam: the bound on the delay that the stable prefix alone does not give.

    Args:
      horizon: None, an int for all utterances, or a list with an int or None per utterance.
    Returns:
      per utterance the list of labels that became final in this call (in stream order; cluster ids stay
      those of the whole stream).  The session keeps them: labels(), nbest() and stable_frames() go on
      answering for everything received.
    """
    n_utt = self._num_utterances
    if horizon is None:
      hz = None
    elif isinstance(horizon, (int, np.integer)) and not isinstance(horizon, bool):
      if horizon < 0:
        raise ValueError('horizon must be non-negative.')
      hz = [int(horizon)] * n_utt
    else:
      if len(horizon) != n_utt:
        raise ValueError('one horizon (or None) per utterance ({} utterances).'.format(n_utt))
      hz = [-1 if x is None else int(x) for x in horizon]
      if any(x < -1 for x in hz):
        raise ValueError('horizon must be non-negative.')
    new, _ = self._decoder.stream_commit(hz)
    out = [self._ids(u, x) for u, x in enumerate(new)]
    for u in range(n_utt):
      if self._retire_at is not None and out[u]:
        at = len(self._final[u])
        self._seen[u].update({c: at + t for t, c in enumerate(out[u])})   # (ascending t: the last appearance stays)
      self._final[u].extend(out[u])
    return out

  @property
  def committed(self):
    """Per utterance, the number of frames committed so far."""
    return [int(x) for x in self._decoder.stream_committed()]

  # ---- speaker retirement

  def _set_retire_policy(self, retire_at, retire_to, cap):
    """The automatic policy's two thresholds, checked (ValueError before any device work)."""
    def whole(x):
      return not isinstance(x, bool) and isinstance(x, (int, np.integer))
    if retire_at is None:
      if retire_to is not None:
        raise ValueError('retire_to needs retire_at.')
      return
    if not whole(retire_at) or retire_at < 1 or (cap is not None and retire_at > cap):
      raise ValueError('retire_at must be an integer in [1, max_clusters = {}].'.format(cap))
    if retire_to is None:
      retire_to = int(retire_at) // 2
    if not whole(retire_to) or not 0 <= retire_to < retire_at:
      raise ValueError('retire_to must be an integer in [0, retire_at).')
    self._retire_at, self._retire_to, self._cap = int(retire_at), int(retire_to), cap

  def _ids(self, u, local):
    """Cluster indices as the library numbers them now -> the ids of the whole stream: index j is the j-th
    non-negative integer that is not a retired id.  Negative entries (no label) stay."""
    values = local.tolist() if isinstance(local, np.ndarray) else [int(v) for v in local]
    gone = self._gone[u] if self._gone is not None else None
    if not gone:
      return values
    top = max(values, default=-1)
    table = _stable_ids(gone, top + 1)
    return [table[v] if v >= 0 else v for v in values]

  def _indices(self, u, ids):
    """Ids of the whole stream -> the library's present indices, ascending (ValueError for a retired or repeated id)."""
    gone = self._gone[u] if self._gone is not None else []
    out = []
    for c in ids:
      if isinstance(c, bool) or not isinstance(c, (int, np.integer)) or c < 0:
        raise ValueError('utterance {}: cluster id {!r} is not a non-negative integer.'.format(u, c))
      if int(c) in gone:
        raise ValueError('utterance {}: cluster {} is already retired.'.format(u, int(c)))
      out.append(int(c) - sum(1 for g in gone if g < int(c)))
    if len(set(out)) != len(out):
      raise ValueError('utterance {}: a cluster id is given twice.'.format(u))
    return sorted(out)

  def _retired(self, result):
    """Book a stream_retire result: the retired indices become ids that are gone.  Returns them per utterance."""
    out = []
    for u, idx in enumerate(result['retired']):
      ids = self._ids(u, idx)
      if ids:
        if self._gone is None:
          self._gone = [[] for _ in range(self._num_utterances)]
        self._gone[u] = sorted(self._gone[u] + ids)
      out.append(ids)
    return out

  def cluster_counts(self):
    """Per utterance (K, retirable): the largest cluster count over the live hypotheses -- how close the
    utterance is to args.max_clusters -- and the ids retire() would accept now.  Changes nothing."""
    result = self._decoder.stream_retire(clusters=[None] * self._num_utterances)
    return [(int(result['K'][u]), self._ids(u, result['retirable'][u])) for u in range(self._num_utterances)]

  def retire(self, utterances=None, clusters=None):
    """Delete clusters that no live hypothesis can still name (uis_stream_retire; extension).

    A cluster is retirable when every live hypothesis has it, none uses it on a frame of the window (the frames
    not yet committed) and none has it as its last label: a speaker last heard before the window.  Retiring it
    gives its room back to the utterance, which can then open a new cluster where it would have hit
    args.max_clusters.  From then on the decode continues as the reference's beam search would from hypotheses
    with that cluster deleted: the ddCRP prior's denominator shrinks by its block count, so for the prior the
    speaker never existed, and if the speaker returns a new cluster with a new id is opened.  Ids the session
    hands out never change and a retired id is never used again.  A session that never committed and was not
    primed has nothing retirable; a dead utterance (cluster cap, emptied beam) is left alone.

    Args:
      utterances: an iterable of utterance indices, or None for all of them.
      clusters: None -- every retirable cluster of `utterances` -- or a list with one iterable of cluster ids (or
        None: nothing) per utterance of the session; utterances must then be None.
    Returns:
      per utterance the list of ids retired by this call.
    Raises:
      ValueError: an index out of range or given twice, an id that is negative, repeated or already retired.
      _capi.HipLibraryError (status UIS_ERR_INVALID_ARG): an id that is not retirable.  The session is then as it was.
    """
    n_utt = self._num_utterances
    if clusters is not None:
      if utterances is not None:
        raise ValueError('utterances and clusters exclude each other: clusters has one entry per utterance.')
      if not isinstance(clusters, (list, tuple)) or len(clusters) != n_utt:
        raise ValueError('one iterable of cluster ids (or None) per utterance ({} utterances).'.format(n_utt))
      idx = [None if c is None else self._indices(u, c) for u, c in enumerate(clusters)]
      return self._retired(self._decoder.stream_retire(clusters=idx))
    which = None
    if utterances is not None:
      which = [0] * n_utt
      for u in utterances:
        if isinstance(u, bool) or not isinstance(u, (int, np.integer)) or not 0 <= int(u) < n_utt:
          raise ValueError('utterance index {!r} is not in [0, {}).'.format(u, n_utt))
        if which[int(u)]:
          raise ValueError('utterance {} is given twice.'.format(int(u)))
        which[int(u)] = 1
    return self._retired(self._decoder.stream_retire(which=which))

  def _keep_under_cap(self, chunks):
    """retire_at given: before a push that could take an utterance to retire_at clusters or more, commit (with the
    session's horizon), query, and retire retirable clusters, least recently heard first, down to retire_to."""
    sizes = _chunk_sizes(chunks)
    n_utt = self._num_utterances
    if len(sizes) != n_utt:
      return   # (stream_push refuses it in its own words)
    if max(sizes, default=0) > self._cap - self._retire_at:
      raise ValueError('a chunk of {} frames is too long for retire_at = {}: every frame can open a cluster, and '
                       'max_clusters - retire_at = {}.'.format(max(sizes), self._retire_at, self._cap - self._retire_at))
    due = [u for u in range(n_utt) if sizes[u] and self._bound[u] >= self._retire_at]
    if due:
      self.commit([self._horizon if u in due else None for u in range(n_utt)])
      counts = self.cluster_counts()
      picks = [None] * n_utt
      for u in due:
        k, able = counts[u]
        if k > self._retire_to and able:
          able.sort(key=lambda c, seen=self._seen[u]: (seen.get(c, -1), c))
          picks[u] = able[:k - self._retire_to]
      if any(picks):
        self.retire(clusters=picks)
      for u in range(n_utt):   # (the query answered for every utterance: each bound starts again from its K)
        self._bound[u] = counts[u][0] - len(picks[u] or ())
      for u in due:
        if self._bound[u] + sizes[u] > self._cap:
          raise RuntimeError('utterance {}: {} speakers are active inside the window and cannot be retired; with {} '
                             'new frames it could pass max_clusters = {}.  Use a larger args.max_clusters or a '
                             'shorter horizon.'.format(u, self._bound[u], sizes[u], self._cap))
    for u in range(n_utt):
      self._bound[u] += sizes[u]

  def restart(self, utterances):
    """End the given utterances and reuse their slots in place (uis_stream_restart; extension).

    Each utterance named hands out its result and is afterwards what it was when the session opened: nothing
    received, nothing committed, one empty hypothesis.  prime, push, commit, labels, nbest, stable_frames and
    committed treat the slot as new; every other utterance's beam is untouched.  This is also how a slot comes
    back that hit the cluster cap or whose beam a non-finite frame emptied.

    Args:
      utterances: an iterable of utterance indices.
    Returns:
      a list with one entry per utterance of the session: (labels, score) for an utterance named -- the labels
      of its WHOLE stream, committed part first, and the best hypothesis' score as a float -- and None for the
      others.  Where labels() would have failed for that utterance alone (cluster cap, emptied beam) labels is
      None; restart does not raise for it.
    Raises:
      ValueError: an index out of range or given twice.
    """
    n_utt = self._num_utterances
    which = [0] * n_utt
    for u in utterances:
      u = self._utterance(u)
      if which[u]:
        raise ValueError('utterance {} is given twice.'.format(u))
      which[u] = 1
    per_utt, scores, overflow, _ = self._decoder.stream_restart(which)
    out = [None] * n_utt
    for u in range(n_utt):
      if not which[u]:
        continue
      window = self._ids(u, per_utt[u])
      dead = bool(overflow[u]) or (len(window) > 0 and window[0] < 0)
      out[u] = (None if dead else self._final[u] + window, float(scores[u]))
      self._final[u] = []
      if self._gone is not None:
        self._gone[u] = []
      if self._bound is not None:
        self._bound[u], self._seen[u] = 0, {}
      if self._names is not None:
        self._names[u] = {}
    return out

  # ---- moving and checkpointing utterances

  def _utterance(self, utterance):
    if isinstance(utterance, bool) or not isinstance(utterance, (int, np.integer)) or not 0 <= int(utterance) < self._num_utterances:
      raise ValueError('utterance index {!r} is not in [0, {}).'.format(utterance, self._num_utterances))
    return int(utterance)

  def export_state(self, utterance):
    """One live utterance as bytes (uis_stream_export; extension): every hypothesis of its beam, its window and
    what this session knows on top -- the labels committed so far and the retired ids.  Changes nothing.  The
    bytes go into import_state of any slot that has received nothing: of this session or of another one (other
    num_utterances, max_frames, max_clusters, persistent or not), in another process or on another GPU, as long as
    the model and args.beam_size are the same.  There the stream continues bit for bit as it would have here.

    Raises:
      ValueError: an index out of range.
      _capi.HipLibraryError: an utterance that has hit the cluster cap (status UIS_ERR_CLUSTER_CAP) or whose beam
        a non-finite frame emptied (UIS_ERR_INVALID_ARG): there is nothing to move, restart() is the way back.
    """
    u = self._utterance(utterance)
    blob = self._decoder.stream_export(u)
    gone = self._gone[u] if self._gone is not None else []
    return blob + _pack_state_trailer(blob, self._final[u], gone)

  def import_state(self, utterance, blob, speaker_names=None):
    """Continue an exported utterance in slot `utterance`, which must have received nothing (uis_stream_import).
    labels(), commit(), nbest(), restart() and retire() hand out the same ids as the source session did, and
    restart() returns the whole stream.  All or nothing.

    speaker_names: the source's speaker_names(utterance) -- names are not serialised; the bindings are.  The slot's
    name table becomes this list (None: empty).

    Raises:
      ValueError: an index out of range, bytes that are not an exported state, a state whose hypotheses bind more
        speaker tags than speaker_names has names (before the library is called).
      _capi.HipLibraryError: the library's refusals (status UIS_ERR_INVALID_ARG: a damaged blob, another model or
        beam size, a window longer than max_frames, a slot that has received frames; UIS_ERR_CLUSTER_CAP: a
        hypothesis with more clusters than this session's max_clusters).  The session is then as it was.
    """
    u = self._utterance(utterance)
    core, final, gone = _unpack_state(blob)
    names = [] if speaker_names is None else list(speaker_names)
    if len(names) > _MAX_KNOWN_SPEAKERS or len(set(names)) != len(names):
      raise ValueError('speaker_names must be at most {} distinct names.'.format(_MAX_KNOWN_SPEAKERS))
    most = _capi.blob_max_tag(core)
    if most > len(names):
      raise ValueError('the state binds speaker tag {} but speaker_names has {} names: pass the source session\'s '
                       'speaker_names(utterance).'.format(most, len(names)))
    self._decoder.stream_import(u, core)
    self._name_tables()[u] = {name: g + 1 for g, name in enumerate(names)}
    self._final[u] = final
    if gone:
      if self._gone is None:
        self._gone = [[] for _ in range(self._num_utterances)]
      self._gone[u] = gone
    elif self._gone is not None:
      self._gone[u] = []
    if self._bound is not None:   # (as after a query: K of the blob; the last committed appearances from the labels)
      self._bound[u] = _capi.blob_info(core)['K']
      self._seen[u] = {c: t for t, c in enumerate(final)}

  def snapshot(self):
    """export_state of every utterance: a list with bytes per utterance, None where an utterance cannot be
    exported (cluster cap, emptied beam).  With restore(): a checkpoint of the whole session."""
    out = []
    for u in range(self._num_utterances):
      try:
        out.append(self.export_state(u))
      except _capi.HipLibraryError as err:
        if getattr(err, 'status', None) not in (_capi.UIS_ERR_CLUSTER_CAP, _capi.UIS_ERR_INVALID_ARG):
          raise
        out.append(None)
    return out

  def restore(self, states):
    """import_state of every entry of a snapshot() into the slot of the same index; None entries are left as
    they are (fresh, in a session that has just been opened)."""
    if not isinstance(states, (list, tuple)) or len(states) != self._num_utterances:
      raise ValueError('one state (or None) per utterance ({} utterances).'.format(self._num_utterances))
    for u, state in enumerate(states):
      if state is not None:
        self.import_state(u, state)

  def labels(self):
    per_utt, _, overflow, _ = self._decoder.stream_labels()
    if overflow.any():
      raise RuntimeError('utterance(s) {} need more than max_clusters clusters per hypothesis; '
                         'open the session with a larger args.max_clusters'.format(
                             np.flatnonzero(overflow).tolist()))
    return [self._final[u] + self._ids(u, x) for u, x in enumerate(per_utt)]

  def _nbest(self, n_best):
    if n_best is None:
      n_best = self._beam_size
    if isinstance(n_best, bool) or not isinstance(n_best, (int, np.integer)):
      raise ValueError('n_best must be an integer in [1, args.beam_size].')
    if not 1 <= int(n_best) <= self._beam_size:
      raise ValueError('n_best must be in [1, args.beam_size = {}].'.format(self._beam_size))
    out = self._decoder.stream_nbest(int(n_best))
    if out['status'] == _capi.UIS_ERR_CLUSTER_CAP:
      self.labels()  # (raises, naming the utterances)
    return out

  def nbest(self, n_best=None):
    """Every hypothesis of the current beam for everything received: per utterance the pair
    (labelings, scores) of UISRNN.predict_nbest; labelings[0] is what labels() returns.  An utterance
    that has received nothing yet has no hypothesis: ([], []).  After commit() the labelings are those of the
    whole stream, committed part first; an utterance whose window a commit emptied has its one hypothesis.

    Cost: a back-trace of every requested rank and a download of n_best labels per frame received.
    In a persistent session the resident launch has to leave the device for it and the next push
    starts a new one (a launch plus the kernel's weight load): read every few pushes, not after each,
    or the session loses most of what persistent=True buys."""
    out = self._nbest(n_best)
    return [([self._final[u] + self._ids(u, row) for row in out['labels'][u][:int(out['counts'][u])]],
             [float(x) for x in out['scores'][u][:int(out['counts'][u])]])
            for u in range(len(out['labels']))]

  def stable_frames(self):
    """Per utterance, the number of leading frames whose labels are final: all hypotheses of the
    beam share them, and every later beam descends from this one.  A guarantee, not a latency
    promise -- a wide beam can keep an early alternative alive for a long time.

    Cost: that of nbest(1) -- the readout runs and the best hypothesis' labels are downloaded -- and,
    like nbest, it makes a persistent session's resident launch leave the device.  Not for polling
    after every push of a persistent session."""
    return [len(self._final[u]) + int(x) for u, x in enumerate(self._nbest(1)['stable'])]

  def posteriors(self, temperature=1.0):
    """The beam's per-frame confidence over the WINDOW -- the frames received and not yet committed (committed
    labels are final) -- as UISRNN.predict_posteriors defines it: per utterance the triple (confidence, change,
    weights), two float32 arrays of the window's length and the float32 weights of the live hypotheses, best first.
    change[0] is 0 also when committed frames precede the window.  An utterance that has received nothing has
    empty arrays; one whose window a commit emptied has no frames and the weights [1].

    Cost: the walks of nbest() and a download of two floats per frame, whatever the beam; like nbest it makes a
    persistent session's resident launch leave the device."""
    temperature = _check_temperature(temperature)
    out = self._decoder.stream_posterior(temperature)
    if out['status'] == _capi.UIS_ERR_CLUSTER_CAP:
      self.labels()  # (raises, naming the utterances)
    return [(out['confidence'][u], out['change'][u], out['weights'][u][:int(out['counts'][u])].copy())
            for u in range(len(out['confidence']))]

  def close(self):
    if self._open:
      self._decoder.stream_end()
      self._decoder.close()
      self._open = False

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    self.close()


class StreamPool:
  """An open-ended set of streams over the slots of ONE OnlineSession (extension).

  A stream is opened under a key and takes a free slot; when it finishes, its labels are handed out and the slot is
  free for the next stream, while the other streams' beams live on (OnlineSession.restart).  One push advances
  every stream that received frames, in one batch.

    with model.online_pool(64, inference_args, max_frames=2000) as pool:
      pool.open('call-17')
      pool.push({'call-17': chunk, 'call-4': other_chunk})
      labels, score = pool.finish('call-17')
  """

  def __init__(self, session):
    self._session = session
    self._slot = {}   # key -> slot
    self._free = list(range(session._num_utterances - 1, -1, -1))  # pylint: disable=protected-access

  def open(self, key, max_speakers=None, min_turn=None):
    """Take a free slot for a new stream.  Returns the slot's index.  max_speakers: None (the slot keeps the bound it
    has), 0 (no bound) or the bound the slot gets for this stream.  min_turn: None (the slot keeps the minimum turn
    length it has) or the value the slot gets for this stream (0 and 1: no rule)."""
    if key in self._slot:
      raise KeyError('stream {!r} is already open'.format(key))
    if not self._free:
      raise RuntimeError('no free slot')
    if min_turn is not None:
      _check_min_turn([min_turn], 1)   # (raises before any device work; 0 and 1 are values too)
    if max_speakers is not None:
      limit = _check_max_speakers([max_speakers], None, 1)
      values = self._session.max_speakers()
      values[self._free[-1]] = limit[0] if limit else 0
      self._session.set_max_speakers(values)
    if min_turn is not None:
      values = self._session.min_turn()
      values[self._free[-1]] = int(min_turn)
      self._session.set_min_turn(values)
    self._slot[key] = self._free.pop()
    return self._slot[key]

  def push(self, chunks, transition_bias=None, known_speakers=None):
    """chunks: a dict {key: [n, D] float64 array} with the new frames of the streams that received some.
    transition_bias: None, a number, or a dict {key: array of the chunk's length} for the streams that have values of
    their own (OnlineSession.push).  known_speakers: None, or a dict {key: sequence of names (None: unknown) of the
    chunk's length} for the streams that have some (OnlineSession.push)."""
    self._per_slot_push(self._session.push, chunks, transition_bias, known_speakers)

  def _per_slot_push(self, push, chunks, transition_bias, known_speakers):
    """push / push_tensors: the dicts by key as the session's lists by slot, then the session's own call."""
    per_slot = [None] * self._session._num_utterances  # pylint: disable=protected-access
    for key, chunk in chunks.items():
      per_slot[self._slot[key]] = chunk
    if isinstance(transition_bias, dict):
      bias_slot = [None] * len(per_slot)
      for key, values in transition_bias.items():
        bias_slot[self._slot[key]] = values
      transition_bias = bias_slot
    if known_speakers is not None:
      if not isinstance(known_speakers, dict):
        raise ValueError('known_speakers of a pool must be a dict {key: sequence of names}.')
      names_slot = [None] * len(per_slot)
      for key, values in known_speakers.items():
        names_slot[self._slot[key]] = values
      known_speakers = names_slot
    push(per_slot, transition_bias, known_speakers)

  def push_tensors(self, chunks, transition_bias=None, known_speakers=None):
    """push with the streams' new frames in device tensors: a dict {key: [n, D] torch tensor}; transition_bias and
    known_speakers as push (OnlineSession.push_tensors)."""
    self._per_slot_push(self._session.push_tensors, chunks, transition_bias, known_speakers)

  def speakers(self, key):
    """{name: label} of the stream's known speakers (OnlineSession.speakers for its slot)."""
    return self._session.speakers()[self._slot[key]]

  def profiles(self, key):
    """The stream's speakers right now (OnlineSession.profiles for its slot): dict(ids, frames, blocks, names, mean), or
    None without a live hypothesis.  The library call answers for every slot of the session at once, so each key pays
    the whole session's query: a caller that wants many keys at one moment reads OnlineSession.profiles() once."""
    return self._session.profiles()[self._slot[key]]

  def speaker_names(self, key):
    """The stream's known speakers in tag order (OnlineSession.speaker_names)."""
    return self._session.speaker_names(self._slot[key])

  def labels(self, key):
    """The currently best labels of everything the stream has received."""
    return self._session.labels()[self._slot[key]]

  def posteriors(self, key, temperature=1.0):
    """(confidence, change, weights) of the stream's window: OnlineSession.posteriors for its slot."""
    temperature = _check_temperature(temperature)
    return self._session.posteriors(temperature)[self._slot[key]]

  def retire(self, key, clusters=None):
    """OnlineSession.retire for the stream's slot: every retirable cluster, or the given ids.  Returns the ids
    retired."""
    slot = self._slot[key]
    if clusters is None:
      return self._session.retire([slot])[slot]
    per_slot = [None] * self._session._num_utterances  # pylint: disable=protected-access
    per_slot[slot] = clusters
    return self._session.retire(clusters=per_slot)[slot]

  def export(self, key):
    """OnlineSession.export_state for the stream's slot.  The key stays open."""
    return self._session.export_state(self._slot[key])

  def adopt(self, key, blob, speaker_names=None):
    """Take a free slot, like open, and continue an exported stream in it (OnlineSession.import_state).  Returns
    the slot's index; a refused blob leaves the pool as it was."""
    slot = self.open(key)
    try:
      self._session.import_state(slot, blob, speaker_names)
    except Exception:
      del self._slot[key]
      self._free.append(slot)
      raise
    return slot

  def finish(self, key):
    """End the stream: (labels, score) of the whole of it (labels None where OnlineSession.restart says so);
    its slot is free afterwards."""
    slot = self._slot[key]
    out = self._session.restart([slot])[slot]
    del self._slot[key]
    self._free.append(slot)
    return out

  def close(self):
    self._session.close()

  def __enter__(self):
    return self

  def __exit__(self, *exc):
    self.close()


def parallel_predict(model, test_sequences, args, num_processes=4, devices=None, max_speakers=None, transition_bias=None,
                     known_speakers=None, min_turn=None):
  """Drop-in for uisrnn.parallel_predict (uisrnn/uisrnn.py:593-623).

  The reference maps utterances over a forkserver process pool.  Here the
  utterances of one GPU are already decoded concurrently in one batch, so the
  workers are GPUs: the list is sharded (longest-processing-time) over
  min(num_processes, visible GPUs) devices, one decoder handle and one host
  thread per device (the C call releases the GIL), no communication during
  decode.  With one GPU this is model.predict.

  Args:
    devices: optional explicit list of HIP device indices (repeats allowed --
      used by the tests to exercise the path on a single-GPU box).
    max_speakers, transition_bias, known_speakers, min_turn: as UISRNN.predict (extensions); every shard takes its
      members' entries.

  Raises:
    TypeError: test_sequences is not a list.
  """
  if not isinstance(test_sequences, list):
    raise TypeError('test_sequences must be a list.')
  _, _, tables = model._offline_arguments(  # pylint: disable=protected-access
      test_sequences, args, max_speakers, transition_bias, known_speakers, sequences_first=True, min_turn=min_turn)
  if not test_sequences:
    return []
  if devices is None:
    n_dev = max(_capi.load_library().uis_device_count(), 1)
    devices = list(range(max(1, min(int(num_processes), n_dev))))
  if len(devices) == 1:
    return model._decode_batch(test_sequences, args, device=devices[0], **tables)  # pylint: disable=protected-access
  import threading  # pylint: disable=import-outside-toplevel
  from uisrnn_amd import distributed  # pylint: disable=import-outside-toplevel
  shards = distributed.shard_utterances(
      [s.shape[0] for s in test_sequences], len(devices))
  # one handle per worker, created up front on this thread (handles are not thread-safe, so
  # a repeated device index gets its own)
  workers = [_Worker(model, device, slot) for slot, device in enumerate(devices)]
  results = [None] * len(test_sequences)
  errors = []

  def run(worker, shard):
    try:
      if shard:
        out = worker.decode([test_sequences[i] for i in shard], args,
                            **{name: None if table is None else [table[i] for i in shard] for name, table in tables.items()})
        for i, labels in zip(shard, out):
          results[i] = labels
    except Exception as exc:  # pylint: disable=broad-except
      errors.append(exc)

  threads = [threading.Thread(target=run, args=(w, sh))
             for w, sh in zip(workers, shards)]
  for thread in threads:
    thread.start()
  for thread in threads:
    thread.join()
  for worker in workers:
    worker.close()
  if errors:
    raise errors[0]
  return results


class _Worker:
  """One decoder handle for one parallel_predict worker thread."""

  def __init__(self, model, device, slot):
    self._model = model
    # the first worker on the model's own device shares the model's handle; every other
    # worker (another device, or the same device again) owns a private one
    self._own = slot > 0 or device != model.device_index
    self._decoder = (_capi.Decoder(model.params, device) if self._own
                     else model._get_decoder(device))  # pylint: disable=protected-access

  def decode(self, sequences, args, limits=None, bias=None, speakers=None, min_turn=None):
    return self._model._decode_batch(  # pylint: disable=protected-access
        sequences, args, decoder=self._decoder, limits=limits, bias=bias, speakers=speakers, min_turn=min_turn)

  def close(self):
    if self._own:
      self._decoder.close()
