"""CPU checks of the sub-cell DOA refinement: the float64 restatement itself, the host-side pieces of
seld_eval.py that need no GPU, and the compiler's resource report of the new kernels."""
import numpy as np
import torch

import seld_eval_ref as ref
import seld_refine_ref as rref


def test_symmetric_map_gives_the_cell_centre():
    """A map that is symmetric around the peak -- the peak alone, or equal weight on mirrored neighbours -- refines to the
    cell centre, away from the poles and at them (where the neighbourhood is one-sided in elevation, so only azimuth
    symmetry holds and only the azimuth is the centre's)."""
    for cell in (9 * 36 + 17, 4 * 36 + 0, 4 * 36 + 35):
        caz, cel = ref.cell_centre(cell)
        alone = np.zeros(648)
        alone[cell] = 0.7
        az, el = rref.refine(alone, cell)
        assert abs(az - caz) <= 1e-5 and abs(el - cel) <= 1e-5
        i, j = divmod(cell, 36)
        sym = alone.copy()
        sym[i * 36 + (j + 1) % 36] = sym[i * 36 + (j - 1) % 36] = 0.2          # the same row: symmetric in azimuth
        az, el = rref.refine(sym, cell)
        assert abs(az - caz) <= 1e-5
        assert abs(el) >= abs(cel) - 1e-9 and abs(el - cel) < 0.5               # the shorter chord lifts it a little
    for cell in (0 * 36 + 5, 17 * 36 + 30):
        m = np.zeros(648)
        for y in rref.neighbourhood(cell):
            m[y] = 0.3
        az, _ = rref.refine(m, cell)
        assert abs(az - ref.cell_centre(cell)[0]) <= 1e-5
    az, el = rref.refine(np.zeros(648), 100)                                    # |v| = 0: the centre itself
    assert (az, el) == tuple(float(v) for v in ref.cell_centre(100))
    nan = np.full(648, np.nan)
    assert rref.refine(nan, 100) == (az, el)


def test_neighbourhood_seam_and_poles():
    """N(x) wraps in azimuth at j = 0 / 35, has 6 cells in the pole rows i = 0 / 17 (no wrap), the centre included, in the
    order di outer, dj inner; a weight across the seam moves the azimuth across it."""
    assert rref.neighbourhood(5 * 36) == [4 * 36 + 35, 4 * 36, 4 * 36 + 1, 5 * 36 + 35, 5 * 36, 5 * 36 + 1,
                                          6 * 36 + 35, 6 * 36, 6 * 36 + 1]
    assert rref.neighbourhood(5 * 36 + 35) == [4 * 36 + 34, 4 * 36 + 35, 4 * 36, 5 * 36 + 34, 5 * 36 + 35, 5 * 36,
                                               6 * 36 + 34, 6 * 36 + 35, 6 * 36]
    assert rref.neighbourhood(0) == [35, 0, 1, 36 + 35, 36, 37]
    assert rref.neighbourhood(17 * 36 + 35) == [16 * 36 + 34, 16 * 36 + 35, 16 * 36, 17 * 36 + 34, 17 * 36 + 35, 17 * 36]
    for cell in range(648):
        assert sorted(rref.neighbourhood(cell)) == sorted([cell] + list(ref.neighbours(cell)))
    m = np.zeros(648)
    m[9 * 36] = 0.5                                   # centre az -175
    m[9 * 36 + 35] = 0.4                              # its neighbour across the seam, az +175
    az, el = rref.refine(m, 9 * 36)
    assert -180.0 <= az < -175.0 and abs(el - 5.0) < 0.1
    m[9 * 36 + 35] = 0.5                              # equal weights: the seam itself, to rounding
    az, _ = rref.refine(m, 9 * 36)
    assert abs(abs(az) - 180.0) < 1e-9 and az != 180.0
    m[9 * 36 + 35] = 0.6
    m[9 * 36] = 0.5
    az, _ = rref.refine(m, 9 * 36 + 35)
    assert 175.0 < az < 180.0


def test_cell_unit_table_is_the_rounded_float64():
    import seld_eval
    t = seld_eval.cell_unit_table()
    assert t.dtype == torch.float32 and tuple(t.shape) == (648, 3)
    assert np.array_equal(t.numpy().astype(np.float64), rref.cell_units())
    assert np.abs(np.linalg.norm(rref.cell_units(fp32=False), axis=1) - 1.0).max() < 1e-15


def test_events_for_segment_with_dirs(tmp_path):
    """dirs= writes rint of the refined degrees, 179.6 -> -180; the CSV round trips through the dataset's reader; dirs=None
    is what it was."""
    import dataset
    import seld_eval
    table = seld_eval.meta_frame_table(np.array([[0, 12], [12, 10]]))
    q_n = len(table)
    assert q_n == 5
    cells = np.full((q_n, 13, 2), -1, np.int32)
    count = np.zeros((q_n, 13), np.int32)
    dirs = np.zeros((q_n, 13, 2, 2), np.float32)
    cells[0, 3, :2], count[0, 3] = (9 * 36 + 35, 40), 2
    dirs[0, 3, 0], dirs[0, 3, 1] = (179.6, 4.4), (-140.5, -79.5)
    cells[2, 0, 0], count[2, 0] = 17 * 36, 1
    dirs[2, 0, 0] = (-179.7, 88.2)
    cells[4, 12, 0], count[4, 12] = 100, 1
    dirs[4, 12, 0] = (179.4, -0.4)
    plain = seld_eval.events_for_segment(cells, count, table, 0)
    assert plain.tolist() == [[0, 3, 0, 175, 5], [0, 3, 1, -135, -75], [2, 0, 0, -175, 85]]
    assert np.array_equal(plain, seld_eval.events_for_segment(cells, count, table, 0, dirs=None))
    got = seld_eval.events_for_segment(cells, count, table, 0, dirs=dirs)
    assert got.dtype == np.int32
    assert got.tolist() == [[0, 3, 0, -180, 4], [0, 3, 1, -140, -80], [2, 0, 0, -180, 88]]     # rint: half to even
    second = seld_eval.events_for_segment(torch.from_numpy(cells), torch.from_numpy(count), table, 1,
                                          dirs=torch.from_numpy(dirs))
    assert second.tolist() == [[1, 12, 0, 179, 0]]
    path = seld_eval.write_events_csv(tmp_path / "e.csv", got)
    assert np.array_equal(dataset._read_metadata_rows(path), got)
    ids = np.full((q_n, 13, 2), -1, np.int32)
    ids[0, 3, :2] = (7, 9)
    ids[2, 0, 0] = 4
    tracked = seld_eval.events_for_segment(cells, count, table, 0, ids=ids, dirs=dirs)
    assert tracked.tolist() == [[0, 3, 7, -180, 4], [0, 3, 9, -140, -80], [2, 0, 4, -180, 88]]


def test_refinement_beats_the_cell_centre_on_synthetic_bumps():
    """One segment of 500 frames (100 meta-frames), three sources of distinct classes per meta-frame, sigma = 6 degree
    bumps of amplitude 0.3, threshold 0.1: all 300 are detected, and the mean refined error is at most a third of the
    mean cell-centre error (the restatement's ratio is about 0.16)."""
    probs, sources = rref.bump_maps(20)
    assert probs.shape == (100, 648, 14) and len(sources) == 300
    n_det, centre, refined = rref.bump_errors(probs, sources)
    print(f"{n_det} detections; cell centre: mean {centre.mean():.3f} max {centre.max():.3f} deg; refined: mean "
          f"{refined.mean():.3f} max {refined.max():.3f} deg; ratio {refined.mean() / centre.mean():.3f}")
    assert n_det == 300 and len(centre) == 300
    assert refined.mean() <= centre.mean() / 3.0
    # the kernel's precision: fp32 products and sums move a direction by far less than the 1e-3 degrees of the GPU test
    worst = 0.0
    for q, c, _, _ in sources[:60]:
        x = int(np.argmax(probs[q, :, c]))
        p32 = probs[q, :, c].astype(np.float32)
        worst = max(worst, float(rref.angle(rref.refine(p32, x), rref.refine(p32, x, fp32_sum=True))))
    print(f"fp32 against float64 summation: {worst:.2e} deg")
    assert worst <= 1e-4


def test_track_dirs_maps_cells_to_directions():
    """One (q, c) with a linked detection and a fill, by hand: the emission whose cell is among the frame's detections
    takes that detection's refined direction whatever its rank, the fill its cell centre, entries past the count 0; a
    detection past det_count is not matched."""
    import seld_eval
    det_cell = torch.full((2, 13, 4), -1, dtype=torch.int32)
    det_count = torch.zeros((2, 13), dtype=torch.int32)
    det_dir = torch.zeros((2, 13, 4, 2), dtype=torch.float32)
    det_cell[0, 5, :2] = torch.tensor([200, 310])
    det_count[0, 5] = 2
    det_dir[0, 5, 0] = torch.tensor([12.25, -33.5])
    det_dir[0, 5, 1] = torch.tensor([-77.0, 3.75])
    det_cell[1, 5, :2] = torch.tensor([201, 310])       # frame 1: the track of cell 310 was not detected (count 1),
    det_count[1, 5] = 1                                  # the stale 310 past the count must not be picked up
    det_dir[1, 5, 0] = torch.tensor([21.5, -31.0])
    det_dir[1, 5, 1] = torch.tensor([99.0, 99.0])
    trk_cell = torch.full((2, 13, 8), -1, dtype=torch.int32)
    trk_count = torch.zeros((2, 13), dtype=torch.int32)
    trk_cell[0, 5, :2] = torch.tensor([310, 200])       # ascending track id, not rank
    trk_count[0, 5] = 2
    trk_cell[1, 5, :2] = torch.tensor([310, 201])       # 310: the fill
    trk_count[1, 5] = 2
    got = seld_eval.track_dirs(trk_cell, trk_count, det_cell, det_count, det_dir)
    assert tuple(got.shape) == (2, 13, 8, 2) and got.dtype == torch.float32
    assert got[0, 5, 0].tolist() == [-77.0, 3.75] and got[0, 5, 1].tolist() == [12.25, -33.5]
    caz, cel = ref.cell_centre(310)
    assert got[1, 5, 0].tolist() == [float(caz), float(cel)] and got[1, 5, 1].tolist() == [21.5, -31.0]
    got[0, 5, :2] = 0
    got[1, 5, :2] = 0
    assert not got.any()
    centres = seld_eval.cell_centre_dirs(torch.arange(648))
    assert np.array_equal(centres.numpy().astype(np.float64), np.stack(ref.cell_centre(np.arange(648)), axis=1))


def test_refine_kernels_do_not_spill():
    """The compiler's own resource report of the refined decode (four instantiations) and the direction matcher shows no
    scratch -- the way test_eval_kernels_do_not_spill checks their parents."""
    from pathlib import Path
    import hip_resources
    csrc = Path(__file__).resolve().parent.parent / "sound-event-localization-detection_amd" / "csrc"
    found = {k: v["scratch"] for k, v in hip_resources.report(csrc / "seld_refine.hip").items()}
    assert len([k for k in found if "refine_decode_kernel" in k]) == 4 and any("doa_match_dirs_kernel" in k for k in found)
    assert all(v == 0 for v in found.values()), found
