"""Plain-Python restatement of the track linking contract -- TEST infrastructure only; the product
(seld_eval.py, csrc/seld_track.hip) never imports it.  Integer arithmetic throughout, so the GPU result must equal this
one entry for entry.  Also the seeded generator of detection lists the GPU test runs on."""
from functools import lru_cache

import numpy as np

import seld_eval_ref as ref

C = 13
SLOTS = 8


@lru_cache(maxsize=None)
def distance_table(i_dim=ref.I, j_dim=ref.J):
    """int32 [I][I][J]: rint(1000 d) for the great-circle angle d (degrees, float64, seld_eval_ref.angle_deg) between the
    centres of cells (i_a, j_a) and (i_b, j_b), indexed (i_a, i_b, (j_b - j_a) mod J)."""
    el = -90.0 + (np.arange(i_dim) + 0.5) * (180.0 / i_dim)
    az = -180.0 + (np.arange(j_dim) + 0.5) * (360.0 / j_dim)
    az1, el1, az2, el2 = np.broadcast_arrays(az[0], el[:, None, None], az[None, None, :], el[None, :, None])
    d = ref.angle_deg(az1, el1, az2, el2)
    return np.rint(1000.0 * d).astype(np.int32)


def dist(table, a, b):
    j_dim = table.shape[2]
    return int(table[a // j_dim, b // j_dim, (b % j_dim - a % j_dim) % j_dim])


def link_chain(frames, table, gate_mdeg, max_gap, min_len):
    """One chain.  ``frames``: list over m of the detection cells in rank order.  Returns (emissions: list over m of
    [(id, cell)] of the kept tracks in ascending id, tracks: [(first_m, last_m, detected, kept)] by id, stats dict)."""
    slots = [None] * SLOTS                               # None or [id, cell, first_m, last_m]
    tracks = []                                          # [first_m, last_m, detected]
    emitted = [[] for _ in frames]                       # (id, cell) per frame, every track
    stats = {"fills": 0, "evictions": 0, "ties": 0, "gate_exact": 0, "max_emissions": 0}
    for m, dets in enumerate(frames):
        for t in range(SLOTS):
            if slots[t] is not None and m - slots[t][3] > max_gap + 1:
                slots[t] = None
        cand = []
        for t in range(SLOTS):
            if slots[t] is None:
                continue
            for r, cell in enumerate(dets):
                d = dist(table, slots[t][1], cell)
                if d <= gate_mdeg:
                    cand.append((d, t, r))
                    stats["gate_exact"] += d == gate_mdeg
        cand.sort()
        ds = [d for d, _, _ in cand]
        stats["ties"] += len(ds) - len(set(ds))
        used_t, used_r = set(), set()
        for d, t, r in cand:
            if t in used_t or r in used_r:
                continue
            used_t.add(t)
            used_r.add(r)
            tid, cell, _, last = slots[t]
            for mm in range(last + 1, m):
                emitted[mm].append((tid, cell))
                stats["fills"] += 1
            slots[t][1], slots[t][3] = dets[r], m
            tracks[tid][1] = m
            tracks[tid][2] += 1
            emitted[m].append((tid, dets[r]))
        for r, cell in enumerate(dets):
            if r in used_r:
                continue
            free = [t for t in range(SLOTS) if slots[t] is None]
            if free:
                t = free[0]
            else:
                t = min((t for t in range(SLOTS) if t not in used_t), key=lambda u: (slots[u][3], u))
                assert slots[t][3] < m
                stats["evictions"] += 1
            slots[t] = [len(tracks), cell, m, m]
            emitted[m].append((len(tracks), cell))
            tracks.append([m, m, 1])
    table_rows = [(f, l, n, int(l - f + 1 >= min_len)) for f, l, n in tracks]
    out = []
    for row in emitted:
        stats["max_emissions"] = max(stats["max_emissions"], len(row))
        out.append(sorted((tid, cell) for tid, cell in row if table_rows[tid][3]))
    stats["removed"] = sum(1 for row in table_rows if not row[3])
    stats["kept_fills"] = sum(len(row) for row in out) - sum(row[2] for row in table_rows if row[3])
    return out, table_rows, stats


def track(det_cell, det_count, seg_offsets, table, gate_mdeg, max_gap, min_len):
    """The five outputs of seld_track_link as numpy arrays, chain_offsets and the summed stats of every chain:
    (trk_cell [Q,13,8], trk_id [Q,13,8], trk_count [Q,13], tracks [T,4], chain_tracks [13 S], chain_offsets [13 S + 1],
    stats).  Rows of ``tracks`` no chain used stay 0."""
    det_cell, det_count = np.asarray(det_cell), np.asarray(det_count)
    q_n, _, k = det_cell.shape
    n_cells = table.shape[0] * table.shape[2]
    seg_offsets = np.asarray(seg_offsets, dtype=np.int64)
    n_seg = len(seg_offsets) - 1
    trk_cell = np.full((q_n, C, SLOTS), -1, np.int32)
    trk_id = np.full((q_n, C, SLOTS), -1, np.int32)
    trk_count = np.zeros((q_n, C), np.int32)
    clamped = np.clip(det_count, 0, k).astype(np.int64)
    per_chain = np.array([clamped[seg_offsets[s]:seg_offsets[s + 1], c].sum() for s in range(n_seg) for c in range(C)],
                         dtype=np.int64)
    chain_offsets = np.concatenate([[0], np.cumsum(per_chain)]).astype(np.int64)
    tracks = np.zeros((int(chain_offsets[-1]), 4), np.int32)
    chain_tracks = np.zeros(n_seg * C, np.int32)
    total = {}
    for s in range(n_seg):
        lo, hi = int(seg_offsets[s]), int(seg_offsets[s + 1])
        for c in range(C):
            frames = []
            for q in range(lo, hi):
                cells = []
                for cell in det_cell[q, c, :int(clamped[q, c])].tolist():
                    if not 0 <= cell < n_cells:
                        break
                    cells.append(cell)
                frames.append(cells)
            out, rows, stats = link_chain(frames, table, gate_mdeg, max_gap, min_len)
            x = s * C + c
            chain_tracks[x] = len(rows)
            if rows:
                tracks[chain_offsets[x]:chain_offsets[x] + len(rows)] = np.array(rows, np.int32)
            for m, row in enumerate(out):
                trk_count[lo + m, c] = len(row)
                for n, (tid, cell) in enumerate(row):
                    trk_id[lo + m, c, n], trk_cell[lo + m, c, n] = tid, cell
            for key, v in stats.items():
                total[key] = max(total.get(key, 0), v) if key == "max_emissions" else total.get(key, 0) + v
    return trk_cell, trk_id, trk_count, tracks, chain_tracks, chain_offsets, total


def synthetic_detections(seg_lengths, k, seed, sources=3, dropout=0.2, clutter=0.35, crowded=0.1, i_dim=ref.I,
                         j_dim=ref.J):
    """Seeded detection lists (det_cell int32 [Q,13,K] with -1 past the count, det_count int32 [Q,13], seg_offsets) for
    segments of ``seg_lengths`` meta-frames.  Per chain: ``sources`` sources that drift by single cells (azimuth wraps,
    elevation clamps), die and are reborn elsewhere now and then, each dropped from a frame with probability
    ``dropout`` and for runs of 2..4 frames now and then; clutter cells at random; a ``crowded`` share of the frames gets
    K + 2 random cells on top (what fills every slot); rank order shuffled, cut to K."""
    rng = np.random.default_rng(seed)
    seg_offsets = np.concatenate([[0], np.cumsum(seg_lengths)]).astype(np.int64)
    q_n = int(seg_offsets[-1])
    det_cell = np.full((q_n, C, k), -1, np.int32)
    det_count = np.zeros((q_n, C), np.int32)
    for s, length in enumerate(seg_lengths):
        for c in range(C):
            pos = [[int(rng.integers(0, i_dim)), int(rng.integers(0, j_dim))] for _ in range(sources)]
            mute = [0] * sources
            for m in range(length):
                cells = []
                for n, p in enumerate(pos):
                    if rng.uniform() < 0.03:
                        p[:] = [int(rng.integers(0, i_dim)), int(rng.integers(0, j_dim))]
                    p[0] = int(np.clip(p[0] + rng.integers(-1, 2), 0, i_dim - 1))
                    p[1] = int((p[1] + rng.integers(-1, 2)) % j_dim)
                    if mute[n] == 0 and rng.uniform() < 0.08:
                        mute[n] = int(rng.integers(2, 5))
                    if mute[n] > 0:
                        mute[n] -= 1
                    elif rng.uniform() >= dropout:
                        cells.append(p[0] * j_dim + p[1])
                while rng.uniform() < clutter:
                    cells.append(int(rng.integers(0, i_dim * j_dim)))
                if rng.uniform() < crowded:
                    cells += [int(x) for x in rng.integers(0, i_dim * j_dim, size=k + 2)]
                cells = list(dict.fromkeys(cells))                       # distinct cells, as the decode gives
                rng.shuffle(cells)
                cells = cells[:k]
                q = int(seg_offsets[s]) + m
                det_count[q, c] = len(cells)
                det_cell[q, c, :len(cells)] = cells
    return det_cell, det_count, seg_offsets


# The GPU test's layout: segments of 70 (crosses a wavefront's 64 lanes), 23, 1 and 0 meta-frames, 52 chains, and its
# settings (K, max_gap, min_len, gate in degrees, generator seed).
GPU_SEGMENTS = (70, 23, 1, 0)
GPU_SETTINGS = ((4, 2, 3, 20.0, 101), (8, 3, 2, 20.0, 102), (8, 0, 1, 14.142, 103), (2, 16, 5, 30.0, 104))


def assert_exercised(stats, k, max_gap, min_len, gate_deg):
    """What a setting's inputs must exercise for the comparison to mean something, from the restatement's own counts."""
    assert stats["max_emissions"] <= SLOTS
    assert stats["ties"] >= 1
    if max_gap > 0:
        assert stats["fills"] >= 1
    if min_len > 1:
        assert stats["removed"] >= 1
    if k == 8:
        assert stats["evictions"] >= 1
    if gate_deg == 20.0:
        assert stats["gate_exact"] >= 1
