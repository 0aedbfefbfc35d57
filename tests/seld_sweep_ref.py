"""Plain-numpy restatement of the threshold sweep of the SELD evaluation -- TEST infrastructure
only; the product (seld_eval.py, csrc/seld_sweep.hip) never imports it.  Nothing here is clever: the prefix tables call
the brute-force matcher of seld_eval_ref on every prefix, the per-threshold metrics call its metrics on the truncated
lists."""
import numpy as np

import seld_eval_ref as ref

C = ref.C
GRID = (0.05, 0.08, 0.1, 0.2, 0.5, 0.9, 0.97)        # the thresholds the tests sweep
SEGMENTS = np.array([[0, 203], [203, 118]])          # 7 windows, 65 meta-frames (41 + 24), both segments end on a partial one
TOTAL = 321
SEED = 3


def leading(scores, threshold):
    """The number of leading entries of ``scores`` (fp32) that reach ``threshold`` (compared in fp32)."""
    n = 0
    for s in np.asarray(scores, dtype=np.float32):
        if not s >= np.float32(threshold):
            break
        n += 1
    return n


def truncate(dets, probs, threshold):
    """decode_detections' lists cut to their leading cells whose P_q reaches ``threshold``."""
    return [[cells[:leading([probs[q, x, c] for x in cells], threshold)] for c, cells in enumerate(row)]
            for q, row in enumerate(dets)]


def prefix_tables(refs, det_cells, det_count, k, thr=20.0):
    """refs: list over (q, c) (row-major) of reference (az, el) lists; det_cells int [Q, 13, K]; det_count int [Q, 13] ->
    (ptp int64 [Q, 13, K + 1], pcost float64 [Q, 13, K + 1]): entry p = seld_eval_ref.match of the first min(p, count)
    detections."""
    q_n = det_count.shape[0]
    ptp = np.zeros((q_n, C, k + 1), np.int64)
    pcost = np.zeros((q_n, C, k + 1))
    for q in range(q_n):
        for c in range(C):
            for p in range(k + 1):
                n = min(p, int(det_count[q, c]))
                _, _, _, tp, cost = ref.match(np.asarray(refs[q * C + c], dtype=np.float64).reshape(-1, 2),
                                              det_cells[q, c, :n], thr)
                ptp[q, c, p], pcost[q, c, p] = tp, cost
    return ptp, pcost


def sweep_metrics(refs, det_cells, det_score, det_count, thresholds, thr=20.0):
    """One seld_eval_ref.metrics record per threshold, on the lists truncated at it."""
    q_n = det_count.shape[0]
    out = []
    for t in thresholds:
        stats = np.zeros((q_n, C, 4), np.int64)
        cost = np.zeros((q_n, C))
        for q in range(q_n):
            for c in range(C):
                n = leading(det_score[q, c, :int(det_count[q, c])], t)
                r, p, k, tp, cst = ref.match(np.asarray(refs[q * C + c], dtype=np.float64).reshape(-1, 2),
                                             det_cells[q, c, :n], thr)
                stats[q, c], cost[q, c] = (r, p, k, tp), cst
        out.append(ref.metrics(stats, cost))
    return out
