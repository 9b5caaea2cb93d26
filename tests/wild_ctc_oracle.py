"""The specification of the CTC loss with a wildcard label (st_ctc_loss_grad_wild_f32, engine.ctc_loss_grad on labels that hold
engine_decode.WILDCARD), float64, in the log domain and safe for -inf logits.  Pure numpy, one utterance at a time.

A label sequence may hold WILDCARD.  It is a label state of the 2L+1 lattice like any other -- blanks around it, at least one
frame, the usual skip rules (it differs from both neighbours, so both skips are open), a label in the "not enough frames" rule
-- whose emission at frame t is

    w_t = e^bias * S_t,      S_t = sum_{c < blank} y_t(c),      bias <= 0 in nats per frame:

the frame reads some label, at a price (the star of Star Temporal Classification, Pratap et al. 2022, without its
minus-next-token refinement).  loss = -ln sum_paths prod emissions, and with occ_t(u) = alpha_t(u) beta_t(u) / p

    d loss / d logit_t(k) = y_t(k) - sum_{u: class(u) = k} occ_t(u) - [k < blank] occ_t(wild) y_t(k) / S_t,

occ_t(wild) the summed occupancy of all wildcard states at t.  Without a wildcard this is tf.nn.ctc_loss."""
import numpy as np

WILDCARD = -1
WILDCARD_BIAS = -1.0


def log_softmax(logits):
  x = np.asarray(logits, dtype=np.float64)
  m = np.max(x, axis=-1, keepdims=True)
  with np.errstate(divide='ignore', invalid='ignore'):
    return x - m - np.log(np.sum(np.exp(x - m), axis=-1, keepdims=True))


def _lse(a, axis=None):
  """log sum exp that returns -inf (not NaN) where everything is -inf."""
  a = np.asarray(a, dtype=np.float64)
  m = np.max(a, axis=axis, keepdims=True)
  m0 = np.where(np.isfinite(m), m, 0.0)
  with np.errstate(divide='ignore'):
    out = m0 + np.log(np.sum(np.exp(a - m0), axis=axis, keepdims=True))
  return np.squeeze(out, axis=axis) if axis is not None else float(out.reshape(()))


def min_frames(label):
  """Frames the label needs: every id, the wildcard included, and a blank between adjacent equal ones."""
  label = list(label)
  return len(label) + sum(label[i] == label[i - 1] for i in range(1, len(label)))


def emissions(logits, label, bias=WILDCARD_BIAS):
  """-> (log y [T, C], log S [T], log emission of every lattice state [T, 2L+1])."""
  ly = log_softmax(logits)
  T, C = ly.shape
  blank = C - 1
  log_s = _lse(ly[:, :blank], axis=1) if T else np.zeros(0)
  em = np.empty((T, 2 * len(label) + 1))
  em[:, 0::2] = ly[:, blank:blank + 1]
  for i, l in enumerate(label):
    em[:, 2 * i + 1] = log_s + bias if l == WILDCARD else ly[:, l]
  return ly, log_s, em


def ctc_loss_and_grad(logits, label, bias=WILDCARD_BIAS):
  """logits [T, C] (any float type, widened), label: ids in [0, C-1) or WILDCARD -> (loss, d loss / d logits [T, C]).
  A label that does not fit its frames: (+inf, zeros), the refusal of the kernels."""
  label = [int(l) for l in label]
  x = np.asarray(logits, dtype=np.float64)
  T, C = x.shape
  blank, L = C - 1, len(label)
  assert all(l == WILDCARD or 0 <= l < blank for l in label) and bias <= 0
  assert not any(a == WILDCARD and b == WILDCARD for a, b in zip(label, label[1:])), 'two adjacent wildcards'
  if min_frames(label) > T:
    return np.inf, np.zeros((T, C))
  if T == 0:
    return 0.0, np.zeros((0, C))
  ly, log_s, em = emissions(x, label, bias)
  U = 2 * L + 1
  skip = np.zeros(U, dtype=bool)                       # state u may be entered from u-2
  for u in range(3, U, 2):
    skip[u] = label[u // 2] != label[u // 2 - 1]
  ninf = -np.inf
  alpha = np.full((T, U), ninf)
  alpha[0, :2] = em[0, :2]
  for t in range(1, T):
    a = alpha[t - 1]
    a1 = np.concatenate([[ninf], a[:-1]])
    a2 = np.where(skip, np.concatenate([[ninf, ninf], a[:-2]]), ninf)
    alpha[t] = _lse(np.stack([a, a1, a2]), axis=0) + em[t]
  beta = np.full((T, U), ninf)                         # excludes the emission at t
  beta[T - 1, max(U - 2, 0):] = 0.0
  skip_up = np.concatenate([skip[2:], [False, False]])   # state u may leave for u+2
  for t in range(T - 2, -1, -1):
    g = beta[t + 1] + em[t + 1]
    g1 = np.concatenate([g[1:], [ninf]])
    g2 = np.where(skip_up, np.concatenate([g[2:], [ninf, ninf]]), ninf)
    beta[t] = _lse(np.stack([g, g1, g2]), axis=0)
  logp = _lse(alpha[T - 1, max(U - 2, 0):])
  if not np.isfinite(logp):
    return np.inf, np.zeros((T, C))
  with np.errstate(invalid='ignore'):
    occ = np.exp(np.where(np.isfinite(alpha) & np.isfinite(beta), alpha + beta - logp, ninf))
  grad = np.exp(ly)
  grad[:, blank] -= occ[:, 0::2].sum(axis=1)
  occ_wild = np.zeros(T)
  for i, l in enumerate(label):
    if l == WILDCARD:
      occ_wild += occ[:, 2 * i + 1]
    else:
      grad[:, l] -= occ[:, 2 * i + 1]
  with np.errstate(invalid='ignore'):
    share = np.where(np.isfinite(log_s)[:, None], np.exp(ly[:, :blank] - np.where(np.isfinite(log_s), log_s, 0.0)[:, None]), 0.0)
  grad[:, :blank] -= np.where(occ_wild[:, None] > 0, occ_wild[:, None] * share, 0.0)
  return float(-logp), grad
