"""Float64 numpy restatement of the weighted / focal cross-entropy class term (csrc/loss_ce.hip, loss.py class_ce_loss).

  target t of a cell: dense labels -> first maximal value (torch.argmax); uint16 mask m -> lowest set bit of m & 0x3fff,
                      background (13) if there is none
  p = softmax(z), q = sum_{c != t} p_c, W = sum_cells w_t
  L = (1/W) sum_cells w_t q^gamma (-log p_t)
  dL/dz_k = grad_scale (w_t / W) f (p_k - [k = t]),  f = q^gamma - gamma p_t q^(gamma-1) log p_t
  a cell with q == 0 contributes 0 to both
"""
import numpy as np

NUM_CLASSES = 14


def mask_targets(mask):
    m = np.asarray(mask).astype(np.int64) & 0x3FFF
    lowest = m & -m                                             # 0 stays 0
    t = np.zeros(m.shape, np.int64)
    nz = lowest != 0
    t[nz] = np.round(np.log2(lowest[nz])).astype(np.int64)      # exact: powers of two up to 2^13
    t[~nz] = NUM_CLASSES - 1
    return t


def dense_targets(dense):
    return np.argmax(np.asarray(dense), axis=-1)               # numpy, like torch: the first maximal value


def targets(labels):
    labels = np.asarray(labels)
    return mask_targets(labels) if labels.dtype == np.uint16 else dense_targets(labels)


def weight_sum(t, weights=None):
    """W = sum_c float64(w_c) * count_c in class order (the counts are integers: exact)."""
    counts = np.bincount(np.asarray(t).reshape(-1), minlength=NUM_CLASSES)
    w = np.ones(NUM_CLASSES) if weights is None else np.asarray(weights, np.float32).astype(np.float64)
    total = 0.0
    for c in range(NUM_CLASSES):
        total += w[c] * float(counts[c])
    return total


def softmax_ce(logits, labels, weights=None, gamma=0.0, grad_scale=1.0):
    """-> (loss, grad [like logits, float64], W).  ``logits``: any float array [..., 14], taken as float64."""
    z = np.asarray(logits, np.float64).reshape(-1, NUM_CLASSES)
    t = targets(labels).reshape(-1)
    n = z.shape[0]
    assert t.shape[0] == n
    w = np.ones(NUM_CLASSES) if weights is None else np.asarray(weights, np.float32).astype(np.float64)
    w_t = w[t]
    big_w = weight_sum(t, weights)
    shifted = z - z.max(axis=1, keepdims=True)
    e = np.exp(shifted)
    denom = e.sum(axis=1)
    p = e / denom[:, None]
    rows = np.arange(n)
    log_pt = shifted[rows, t] - np.log(denom)
    p_t = p[rows, t]
    others = p.copy()
    others[rows, t] = 0.0
    q = others.sum(axis=1)                                      # not 1 - p_t
    live = q > 0
    if gamma == 0.0:
        factor = np.ones(n)
        f = np.ones(n)
    else:
        q_safe = np.where(live, q, 1.0)
        q_gm1 = q_safe ** (gamma - 1.0)
        factor = q_gm1 * q_safe
        f = factor - gamma * p_t * q_gm1 * log_pt
    cell = np.where(live, w_t * factor * -log_pt, 0.0)
    f = np.where(live, f, 0.0)
    onehot = np.zeros_like(p)
    onehot[rows, t] = 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        loss = cell.sum() / big_w
        grad = (grad_scale * w_t * f / big_w)[:, None] * (p - onehot)
    return float(loss), grad.reshape(np.asarray(logits).shape), big_w
