"""Plain-Python / numpy float64 restatement of the segment-based, class-macro SELD metrics with jackknife intervals
 -- TEST infrastructure only; the product (seld_eval.py, csrc/seld_segment.hip) never imports it.
Nothing here is clever: the dp and its tie rule are written out as section 18.1 states them, the rest is loops."""
import math
from itertools import permutations

import numpy as np

import seld_eval_ref as ref

C = ref.C
SLOTS = 8                  # references per (q, c) the matcher takes
BLOCK = 10                 # meta-frames per block
NAN = float("nan")
THR = 20.0 + 1e-6          # what the host hands the kernels for a 20-degree threshold
# the timeline of the kernel tests: 3 recordings of 23, 10 and 7 meta-frames = 40 meta-frames, 5 blocks (3 + 1 + 1), one partial
META = (23, 10, 7)
SEG_OFFSETS = np.array([0, 23, 33, 40], dtype=np.int64)
SEEDS = {4: 65, 8: 68}     # per K: seeds of random_timeline without a near tie of assignments or a slot average at the threshold
# the 0.975 quantiles of Student's t the host's student_t_975 is held to (df -> t)
T975 = {1: 12.706204736432095, 2: 4.302652729696142, 3: 3.182446305284263, 5: 2.570581835636314,
        10: 2.2281388519649385, 30: 2.0422724563012373, 100: 1.9839715184496334}


# ---------------------------------------------------------------------------------------------- per-frame assignment

def distances(ref_dirs, det_dirs):
    """References (az, el) [R, 2] and detections (az, el) [P, 2], degrees -> d [R][P] float64."""
    ref_dirs = np.asarray(ref_dirs, dtype=np.float64).reshape(-1, 2)
    det_dirs = np.asarray(det_dirs, dtype=np.float64).reshape(-1, 2)
    if not (len(ref_dirs) and len(det_dirs)):
        return np.zeros((len(ref_dirs), len(det_dirs)))
    return ref.angle_deg(ref_dirs[:, None, 0], ref_dirs[:, None, 1], det_dirs[None, :, 0], det_dirs[None, :, 1])


def assign(dist):
    """dist [R][P] -> (slots: 8 floats, slot r = the distance of reference r to its detection or nan; total: the dp's
    minimum, added in the dp's order; pairs: [(reference, detection)] in row order)."""
    dist = np.asarray(dist, dtype=np.float64)
    nr, npred = dist.shape
    slots = [NAN] * SLOTS
    refs_are_rows = nr <= npred
    d = dist if refs_are_rows else dist.T
    k, cols = d.shape
    if k == 0:
        return slots, 0.0, []
    dp, choice = {0: 0.0}, {}
    best, best_mask = math.inf, None
    for mask in range(1, 1 << cols):
        pc = bin(mask).count("1")
        if pc > k:
            continue
        row = pc - 1
        v, pick = math.inf, None
        for b in range(cols):
            if not (mask >> b) & 1:
                continue
            cand = dp[mask ^ (1 << b)] + float(d[row, b])
            if cand < v:
                v, pick = cand, b
        dp[mask], choice[mask] = v, pick
        if pc == k and v < best:
            best, best_mask = v, mask
    pairs, mask = [], best_mask
    for row in range(k - 1, -1, -1):
        b = choice[mask]
        pairs.append((row, b) if refs_are_rows else (b, row))
        mask ^= 1 << b
    pairs.reverse()
    for r, p in pairs:
        slots[r] = float(dist[r, p])
    return slots, best, pairs


def assignment_gap(dist):
    """The difference between the cheapest and the second cheapest DISTINCT assignment of the smaller side into the larger
    (brute force); inf when there is only one."""
    dist = np.asarray(dist, dtype=np.float64)
    d = dist if dist.shape[0] <= dist.shape[1] else dist.T
    k, cols = d.shape
    if k == 0:
        return math.inf
    costs = sorted(sum(float(d[row, b]) for row, b in enumerate(inj)) for inj in permutations(range(cols), k))
    return costs[1] - costs[0] if len(costs) > 1 else math.inf


def pair_dist(refs, det_dirs, det_count, k):
    """refs: list over (q, c) (row-major) of reference (az, el) lists; det_dirs float [Q, 13, K, 2] degrees; det_count int
    [Q, 13] -> (pair_dist float64 [Q, 13, 8], totals float64 [Q, 13], pairs: list over (q, c), gaps float64 [Q, 13]).  An
    entry the matcher refuses (more than 8 references, a count outside 0..K) is nan throughout."""
    q_n = det_count.shape[0]
    out = np.full((q_n, C, SLOTS), NAN)
    totals = np.full((q_n, C), NAN)
    gaps = np.full((q_n, C), math.inf)
    pairs = []
    for q in range(q_n):
        for c in range(C):
            rows, n = refs[q * C + c], int(det_count[q, c])
            if len(rows) > SLOTS or n < 0 or n > k:
                pairs.append(None)
                continue
            dist = distances(rows, det_dirs[q, c, :n])
            out[q, c], totals[q, c], pr = assign(dist)
            gaps[q, c] = assignment_gap(dist)
            pairs.append(pr)
    return out, totals, pairs, gaps


def cell_dirs(det_cell):
    """Cells int [...] -> their centres float64 [..., 2]."""
    return np.stack(ref.cell_centre(np.maximum(np.asarray(det_cell), 0)), -1)


def row_order_sum(slots, pairs):
    """The slots of one entry added in the matcher's row order (ascending reference when the references are the rows,
    ascending detection otherwise), from 0.0: what its cost is, bit for bit."""
    total = 0.0
    for r, _ in pairs:
        total = total + float(slots[r])
    return total


# ---------------------------------------------------------------------------------------------- blocks

def block_offsets(seg_offsets):
    frames = np.diff(np.asarray(seg_offsets, dtype=np.int64))
    return np.concatenate([[0], np.cumsum((frames + BLOCK - 1) // BLOCK)]).astype(np.int64)


def block_class(frames, thr=THR):
    """frames: [(R_m, P_m, slots)] of one (block, class) in ascending m -> ((Nref, Npred, TP, FPs, FP, FN, DE_TP, DE_FN), de,
    averages: {slot: average})."""
    nref = max((f[0] for f in frames), default=0)
    npred = max((f[1] for f in frames), default=0)
    sums, cnts = [0.0] * SLOTS, [0] * SLOTS
    for rm, pm, slots in frames:
        if rm > 0 and pm > 0:
            for r in range(SLOTS):
                if not math.isnan(slots[r]):
                    sums[r] += float(slots[r])
                    cnts[r] += 1
    tp = fps = fp = fn = de_tp = de_fn = 0
    de, averages = 0.0, {}
    for r in range(SLOTS):
        if cnts[r] > 0:
            avg = sums[r] / cnts[r]
            averages[r] = avg
            de += avg
            de_tp += 1
            if avg <= thr:
                tp += 1
            else:
                fps += 1
    if nref > 0 and npred > 0:
        if de_tp > 0:
            fp += max(0, npred - nref)
            fn += max(0, nref - npred)
            de_fn += max(0, nref - npred)
        else:
            fn += nref
            de_fn += nref
            fp += npred
    elif nref > 0:
        fn += nref
        de_fn += nref
    else:
        fp += npred
    return (nref, npred, tp, fps, fp, fn, de_tp, de_fn), de, averages


def segment_score(pairs, ref_count, det_count, k, seg_offsets, thr=THR):
    """pair_dist [Q, 13, 8], ref_count / det_count int [Q, 13] -> (seg_stats int64 [NB, 13, 8], seg_de [NB, 13], rec_counts
    int64 [S, 13, 11], rec_sdi int64 [S, 3], rec_de [S, 13], averages: every slot average, for the margin check)."""
    offs = block_offsets(seg_offsets)
    n_seg, n_blocks = len(offs) - 1, int(offs[-1])
    seg_stats = np.zeros((n_blocks, C, 8), np.int64)
    seg_de = np.zeros((n_blocks, C))
    rec_counts = np.zeros((n_seg, C, 11), np.int64)
    rec_sdi = np.zeros((n_seg, 3), np.int64)
    rec_de = np.zeros((n_seg, C))
    averages = []
    for s in range(n_seg):
        lo, hi = int(seg_offsets[s]), int(seg_offsets[s + 1])
        for x in range(int(offs[s + 1] - offs[s])):
            b = int(offs[s]) + x
            q0, q1 = lo + BLOCK * x, min(lo + BLOCK * x + BLOCK, hi)
            loc_fp_all = loc_fn_all = 0
            for c in range(C):
                frames = [(int(ref_count[q, c]), min(max(int(det_count[q, c]), 0), k), pairs[q, c]) for q in range(q0, q1)]
                stats, de, avgs = block_class(frames, thr)
                averages.extend(avgs.values())
                seg_stats[b, c], seg_de[b, c] = stats, de
                loc_fp, loc_fn = stats[3] + stats[4], stats[5]
                rec_counts[s, c, :8] += stats
                rec_counts[s, c, 8] += min(loc_fp, loc_fn)
                rec_counts[s, c, 9] += max(0, loc_fn - loc_fp)
                rec_counts[s, c, 10] += max(0, loc_fp - loc_fn)
                rec_de[s, c] += de
                loc_fp_all += loc_fp
                loc_fn_all += loc_fn
            rec_sdi[s] += (min(loc_fp_all, loc_fn_all), max(0, loc_fn_all - loc_fp_all), max(0, loc_fp_all - loc_fn_all))
    return seg_stats, seg_de, rec_counts, rec_sdi, rec_de, averages


# ---------------------------------------------------------------------------------------------- metrics

def figures(nref, tp, fps, fp, fn, de_tp, de_fn, sdi, de):
    """(F, ER, LE, LR, SELD) of one set of counts; empty denominators give nan, LE is 180 when DE_TP = 0."""
    f_den = (tp + fps) + 0.5 * (fp + fn)
    f = tp / f_den if f_den else NAN
    er = sdi / nref if nref else NAN
    le = de / de_tp if de_tp else 180.0
    lr = de_tp / (de_tp + de_fn) if de_tp + de_fn else NAN
    return [f, er, le, lr, (er + (1.0 - f) + le / 180.0 + (1.0 - lr)) / 4.0]


def metrics(rec_counts, rec_sdi, rec_de, keep):
    """The recordings ``keep`` (ascending) -> (micro [5], macro [5], per_class [13][5])."""
    tot, tot_de, per_class, macro, n_classes = [0] * 8, 0.0, [], [0.0] * 5, 0
    for c in range(C):
        acc, de = [0] * 11, 0.0
        for s in keep:
            acc = [a + int(v) for a, v in zip(acc, rec_counts[s, c])]
            de += float(rec_de[s, c])
        f = figures(acc[0], acc[2], acc[3], acc[4], acc[5], acc[6], acc[7], acc[8] + acc[9] + acc[10], de)
        per_class.append(f)
        if acc[0] > 0:
            n_classes += 1
            macro = [m + v for m, v in zip(macro, f)]
        tot = [t + a for t, a in zip(tot, acc[:8])]
        tot_de += de
    sdi = sum(int(rec_sdi[s].sum()) for s in keep)
    micro = figures(tot[0], tot[2], tot[3], tot[4], tot[5], tot[6], tot[7], sdi, tot_de)
    return micro, [m / n_classes if n_classes else NAN for m in macro], per_class


def jackknife_rows(rec_counts, rec_sdi, rec_de):
    """out [S + 1][2][5]: row j leaves recording j out, row S none; and the per-class figures of row S."""
    n_seg = rec_counts.shape[0]
    out = np.zeros((n_seg + 1, 2, 5))
    per_class = None
    for j in range(n_seg + 1):
        micro, macro, per_class = metrics(rec_counts, rec_sdi, rec_de, [s for s in range(n_seg) if s != j])
        out[j, 0], out[j, 1] = micro, macro
    return out, np.array(per_class)


def jackknife(replicates, full, t):
    """The delete-one jackknife of one figure, with ``t`` the 0.975 quantile of Student's t with (usable n) - 1 degrees of
    freedom, given by the caller: (estimate, bias, se, low, high, n)."""
    rep = [float(v) for v in replicates if not math.isnan(v)]
    n = len(rep)
    if n < 2:
        return full, NAN, NAN, NAN, NAN, n
    mean = sum(rep) / n
    bias = (n - 1) * (mean - full)
    se = math.sqrt((n - 1) / n * sum((v - mean) ** 2 for v in rep))
    estimate = full - bias
    return estimate, bias, se, estimate - t * se, estimate + t * se, n


# ---------------------------------------------------------------------------------------------- seeded kernel inputs

def random_timeline(k, seed):
    """The inputs of the kernel tests on the META timeline: (det_cell int32 [40, 13, K], det_dir f32 [40, 13, K, 2],
    det_count int32 [40, 13], offsets int32 [40 * 13 + 1], dirs int32 [R, 2], refs: list per entry).  0..K detections on
    distinct cells and 0..3 integer references per (q, c), about a third of the entries empty on either side, references
    near a detection (within 24 degrees per axis: on both sides of the threshold) more often than not; class 11 has
    references only, class 12 detections only."""
    rng = np.random.default_rng(seed)
    q_n = int(SEG_OFFSETS[-1])
    cell = np.full((q_n, C, k), -1, np.int32)
    count = np.zeros((q_n, C), np.int32)
    refs = []
    for q in range(q_n):
        for c in range(C):
            p = 0 if c == 11 or rng.uniform() < 0.3 else int(rng.integers(1, k + 1))
            cell[q, c, :p] = rng.choice(ref.I * ref.J, size=p, replace=False)
            count[q, c] = p
            rows = []
            n_refs = 0 if c == 12 or rng.uniform() < 0.3 else int(rng.integers(1, 4))
            for _ in range(n_refs):
                if p and rng.uniform() < 0.7:
                    caz, cel = ref.cell_centre(cell[q, c, int(rng.integers(0, p))])
                    rows.append((int(np.clip(caz + rng.integers(-24, 25), -180, 180)),
                                 int(np.clip(cel + rng.integers(-24, 25), -90, 90))))
                else:
                    rows.append((int(rng.integers(-180, 181)), int(rng.integers(-90, 91))))
            refs.append(rows)
    det_dir = cell_dirs(cell).astype(np.float32) + rng.uniform(-4.0, 4.0, size=(q_n, C, k, 2)).astype(np.float32)
    det_dir[..., 1] = np.clip(det_dir[..., 1], -90.0, 90.0)
    det_dir[np.arange(k) >= count[..., None]] = 0.0
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in refs])]).astype(np.int32)
    dirs = np.array([d for r in refs for d in r], np.int32).reshape(-1, 2)
    return cell, det_dir, count, offsets, dirs, refs
