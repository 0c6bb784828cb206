"""Right-camera samples (DATASETS.USE_RIGHT_IMAGE) without a GPU: the right-view restatement against the reference's goldens,
the device functions compiled for the host (tests/shim/kitti_encode_views_host.cpp) against the goldens and the restatement,
and the dataset front (length, files, calibration, view flag, split handling) on a generated KITTI directory."""
import random

import numpy as np
import pytest
import torch

from monoflex_amd import synthetic as S
from monoflex_amd.data import encode as E
from oracle import kitti_encode_ref as K
from tests import kitti_right_common as R
from tests.kitti_common import GOLD, NAMES, compare_fields, golden_sample

LEFT_FIELDS = R.GOLD_FIELDS


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return R.build_views_shim(tmp_path_factory.mktemp("views_shim"))


def test_fixture_is_the_recorded_condition():
    """What the recorder saw in the reference: 24 samples, s03 and s11 raise, ten cases with 75 kept objects, three flipped ones with objects."""
    assert int(R.GOLD_R["len"]) == 2 * len(R.NAMES_R) == 24 and R.NAMES_R == NAMES
    assert np.array_equal(R.GOLD_R["P3"], S.KITTI_P3) and np.array_equal(S.KITTI_P3[:, :3], S.KITTI_P2[:, :3])
    assert R.RAISED == ["s03", "s11"] and all("TypeError" in str(R.GOLD_R[n + "_error"]) for n in R.RAISED)
    kept = [int(R.GOLD_R[n + "_reg_mask"].sum()) for n in R.KEPT]
    assert kept == [4, 0, 9, 7, 0, 25, 8, 2, 14, 6] and sum(kept) == 75
    flipped = [n for n in R.KEPT if R.golden_right_sample(n)[3] and R.GOLD_R[n + "_reg_mask"].sum() > 0]
    assert flipped == ["s06", "s07", "s09"]
    for n in R.KEPT:                                                   # same label text as the left-view fixture; every kept box differs from it
        assert str(R.GOLD_R[n + "_labels"]) == str(GOLD[n + "_labels"])
        both = (R.GOLD_R[n + "_reg_mask"] > 0) & (GOLD[n + "_reg_mask"] > 0)
        assert (R.GOLD_R[n + "_gt_bboxes"][both] != GOLD[n + "_gt_bboxes"][both]).any(axis=1).all()


def test_restatement_reproduces_the_reference_goldens():
    for n in R.KEPT:
        lines, w, h, flip, _ = R.golden_right_sample(n)
        got = R.encode_right_sample(lines, R.P3, w, h, do_flip=flip)
        compare_fields(got, R.golden_right_fields(n), n)
        np.testing.assert_allclose(got["P"], R.GOLD_R[n + "_P"], rtol=0, atol=1e-12)
    for n in R.RAISED:
        lines, w, h, flip, _ = R.golden_right_sample(n)
        with pytest.raises(TypeError):
            R.encode_right_sample(lines, R.P3, w, h, do_flip=flip)
    assert K.read_objects.__module__ == K.__name__ and K.read_objects.__name__ == "read_objects"      # the substitution was undone


def test_shim_matches_right_view_goldens_as_one_batch(shim):
    samples = [R.golden_right_sample(n)[:4] for n in R.NAMES_R]
    out = R.run_views_shim(shim, samples, [1] * len(samples))
    for b, n in enumerate(R.NAMES_R):
        if n in R.RAISED:
            assert out["status"][b] != 0, n
            continue
        assert out["status"][b] == 0, n
        compare_fields({k: v[b] for k, v in out.items()}, R.golden_right_fields(n), n)
        for k in ("gt_bboxes", "2d_bboxes"):                            # the regenerated box and its float32 flip chain: bit for bit
            assert np.array_equal(out[k][b], R.GOLD_R[n + "_" + k]), (n, k)
        np.testing.assert_allclose(out["P"][b], R.GOLD_R[n + "_P"], rtol=0, atol=1e-12)


def test_shim_left_view_rows_did_not_move(shim):
    """right = 0 (and no flag array at all) still gives the left-view goldens, and the same bytes as each other."""
    samples = [golden_sample(n)[:4] for n in NAMES]
    zeros, none = R.run_views_shim(shim, samples, [0] * len(samples)), R.run_views_shim(shim, samples, None)
    assert (zeros["status"] == 0).all()
    for k in zeros:
        assert zeros[k].tobytes() == none[k].tobytes(), k
    for b, n in enumerate(NAMES):
        compare_fields({k: v[b] for k, v in zeros.items()}, {k: GOLD[n + "_" + k] for k in LEFT_FIELDS}, n)
        np.testing.assert_allclose(zeros["P"][b], GOLD[n + "_P"], rtol=0, atol=1e-12)


def test_shim_matches_restatement_on_mixed_fuzzed_batches(shim):
    """The seed set and the cap of the GPU test (fuzz_sample(1000 .. 1299), every seed as a left-view and a right-view row): every
    left-view row and at least half of the right-view rows are compared; rows the restatement raises on must flag a status."""
    samples, rights, refs = R.mixed_fuzz_batch(R.FUZZ_SEEDS)
    compared, per = {0: 0, 1: 0}, 60
    for lo in range(0, len(samples), per):
        out = R.run_views_shim(shim, samples[lo:lo + per], rights[lo:lo + per])
        for b, ref in enumerate(refs[lo:lo + per]):
            if ref is None:
                assert out["status"][b] != 0, lo + b
                continue
            assert out["status"][b] == 0, lo + b
            compare_fields({k: v[b] for k, v in out.items()}, ref, "fuzz%d" % (lo + b))
            compared[rights[lo + b]] += 1
    n = len(R.FUZZ_SEEDS)
    print("compared: left %d / %d, right %d / %d" % (compared[0], n, compared[1], n))
    assert n == 300 and compared[0] == n and 2 * compared[1] >= n, compared
    combos = {(r, f) for (_, _, _, f), r, ref in zip(samples, rights, refs) if ref is not None}
    assert combos == {(0, False), (0, True), (1, False), (1, True)}


def test_regenerated_boxes_equal_the_restatement_bit_for_bit(shim):
    """right_view_box alone against the restatement's float32 box, every object of the first 40 fuzz seeds."""
    from tests.kitti_common import fuzz_sample
    n = 0
    for seed in range(1000, 1040):
        lines, w, h, _ = fuzz_sample(seed)
        kept = [l for l in lines if l.split(" ")[0] in R.CLASSES]
        for line, o in zip(kept, R.right_view_objects(lines, R.P3, w, h)):
            assert np.array_equal(R.shim_right_view_box(shim, line, R.P3, w, h), o.box2d, equal_nan=True), (seed, line)
            n += 1
    assert n > 300


def test_corners_at_zero_depth_are_clamped_like_python_max(shim):
    """Corners with zero depth project to +-inf (x / 0); Python's max / min clamp them into the image and no object is dropped at
    that stage: the restatement and the device functions agree on such an object, flipped or not."""
    P = R.P3.copy(); P[2, 3] = 0.0
    line = "Car 0.30 0 1.50 100.00 150.00 400.00 250.00 1.50 2.00 4.00 -2.00 1.65 1.00 0.00"    # w/2 == tz: four corners at depth 0
    objs = R.right_view_objects([line], P, 1242, 375)
    assert np.isfinite(objs[0].box2d).all() and np.array_equal(R.shim_right_view_box(shim, line, P, 1242, 375), objs[0].box2d)
    for flip in (False, True):
        ref = R.right_oracle_fields([line], 1242, 375, flip, P=P)
        recs = [R.KU.read_label_records([line], R.CLASSES)]
        out = R.shim_encode_records(shim, recs, [P], [(1242, 375)], [flip], E.EncodeParams(), [1])
        if ref is None:
            assert out["status"][0] != 0
        else:
            assert out["status"][0] == 0
            compare_fields({k: v[0] for k, v in out.items()}, ref, "plane flip=%s" % flip)


def test_a_nan_corner_passes_through_like_numpy_min_and_python_max(shim):
    """A corner on the camera plane whose numerator is zero as well projects to 0 / 0 = NaN. numpy's .min() / .max() hand the NaN
    on and so does Python's `max(nan, 0)` / `min(nan, w - 1)`: the regenerated box has NaN in xmin and xmax, in the restatement and
    in the device functions alike, while ymin / ymax come from the +-inf of the same corners. The object is not dropped there; it
    goes on and fails `(bbox_dim > 0).all()` later, without a status."""
    P = R.P3.copy(); P[2, 3] = 0.0; P[0, 3] = 0.0
    # ry = 0, l = 1, w = 2, t = (-0.5, 0.8, 1): the corners (+l/2, ., -w/2) sit at X = 0, Z = 0 -> u = 0 / 0; the 3D centre projects inside the image
    line = "Car 0.00 0 1.50 100.00 150.00 400.00 250.00 1.50 2.00 1.00 -0.50 0.80 1.00 0.00"
    (o,) = R.right_view_objects([line], P, 1242, 375)
    assert np.isnan(o.box2d[[0, 2]]).all() and o.box2d[1] == 0 and o.box2d[3] == 374
    got = R.shim_right_view_box(shim, line, P, 1242, 375)
    assert np.array_equal(got, o.box2d, equal_nan=True) and np.isnan(got[[0, 2]]).all()
    for flip in (False, True):
        ref = R.encode_right_sample([line], P, 1242, 375, do_flip=flip)              # the reference's arithmetic does not raise on it
        out = R.shim_encode_records(shim, [R.KU.read_label_records([line], R.CLASSES)], [P], [(1242, 375)], [flip], E.EncodeParams(), [1])
        assert out["status"][0] == 0 and out["reg_mask"][0].sum() == 0 == ref["reg_mask"].sum()
        compare_fields({k: v[0] for k, v in out.items()}, ref, "nan flip=%s" % flip)


# ---- dataset front -----------------------------------------------------------------------------------------------------
CASES = [(S.synthetic_kitti_labels(40 + i, w, h, 9), w, h) for i, (w, h) in enumerate([(1242, 375), (1224, 370), (1238, 374)])]


def test_dataset_front_with_right_images(tmp_path):
    from monoflex_amd.config import get_cfg
    from monoflex_amd.data import KITTIDataset
    root = R.make_kitti_dir(tmp_path / "kitti", CASES, splits=("train", "val"))
    N = len(CASES)
    ds = KITTIDataset(R.right_cfg(), root, is_train=True, augment=False)
    assert ds.use_right_img and len(ds) == 2 * N and ds.num_samples == N and ds.image_right_dir.endswith("image_3")
    for i, (lines, w, h) in enumerate(CASES):
        left, right = ds.load_raw(i), ds.load_raw(N + i)
        assert left.right is False and right.right is True and left.original_idx == right.original_idx == "%06d" % i
        assert np.array_equal(left.frame, R.frame_pixels(R.left_frame_seed(i), w, h))
        assert np.array_equal(right.frame, R.frame_pixels(R.right_frame_seed(i), w, h))
        assert np.allclose(left.calib.P, S.KITTI_P2, rtol=0, atol=1e-9) and np.allclose(right.calib.P, R.P3, rtol=0, atol=1e-9)
        assert np.array_equal(left.records, right.records) and right.flip is False
    for bad in (2 * N, 2 * N + 1, -2 * N - 1):
        with pytest.raises(IndexError):
            ds.load_raw(bad)
    for idx in (np.int64(N + 1), torch.tensor(N + 1)):                 # what a sampler may yield: the flag stays a Python bool
        raw = ds.load_raw(idx)
        assert raw.right is True and raw.original_idx == "000001"
    assert ds.load_raw(np.int64(1)).right is False
    last = ds.load_raw(-1)                                             # from the end, as a sequence: the last right-view sample
    assert last.right is True and last.original_idx == "%06d" % (N - 1) and ds.load_raw(-N - 1).right is False
    # the flip coin is tossed for right-view samples as for left-view ones
    coin = KITTIDataset(R.right_cfg(), root, is_train=True)
    random.seed(0)
    assert 8 < sum(coin.load_raw(N + 1).flip for _ in range(40)) < 32
    # is_train=False masks the setting; the setting off keeps today's dataset
    val = KITTIDataset(R.right_cfg(), root, is_train=False)
    assert not val.use_right_img and len(val) == N
    with pytest.raises(IndexError):
        val.load_raw(N)
    import os
    off = KITTIDataset(get_cfg(os.path.join(R.ROOT, "runs", "monoflex.yaml")), root, is_train=True)
    assert not off.use_right_img and len(off) == N
    with pytest.raises(IndexError):
        off.load_raw(N)


def test_missing_image_3_is_named(tmp_path):
    from monoflex_amd.data import KITTIDataset
    root = R.make_kitti_dir(tmp_path / "kitti", CASES, splits=("train", "val"), right_images=False)
    with pytest.raises(FileNotFoundError, match="image_3"):
        KITTIDataset(R.right_cfg(), root, is_train=True)
    assert len(KITTIDataset(R.right_cfg(), root, is_train=False)) == len(CASES)        # not needed where the setting is masked


def test_config_file_line_switches_it_on(tmp_path):
    """The user's own copy of the reference's right-view experiment file: runs/monoflex.yaml plus one line."""
    import os
    from monoflex_amd.config import get_cfg
    from monoflex_amd.data import KITTIDataset
    text = open(os.path.join(R.ROOT, "runs", "monoflex.yaml")).read()
    assert "USE_RIGHT_IMAGE: False" in text
    mine = tmp_path / "monoflex_right.yaml"
    mine.write_text(text.replace("USE_RIGHT_IMAGE: False", "USE_RIGHT_IMAGE: True"))
    root = R.make_kitti_dir(tmp_path / "kitti", CASES)
    assert len(KITTIDataset(get_cfg(str(mine)), root, is_train=True)) == 2 * len(CASES)


def test_dataset_targets_equal_the_reference_fixture_on_cpu(tmp_path, shim, monkeypatch):
    """KITTIDataset end to end with the two GPU launches replaced by the host build of the same device functions: ds[N + i] on a
    folder holding the fixture's label sets gives the fixture's targets, calib and right-camera frame; mixed batches keep rows apart."""
    import monoflex_amd.data.datasets.kitti as DK
    from monoflex_amd.data import KITTIDataset

    def encode(records, Ps, sizes, flips, params, device, check=True, rights=None):
        out = {k: torch.from_numpy(v) for k, v in R.shim_encode_records(shim, records, Ps, sizes, flips, params, rights).items()}
        if check:
            E.check_status(out["status"])
        return out

    def frames(fr, flips, params, device, mean, std):
        return torch.from_numpy(np.stack([K.transform_image(f, bool(fl)) for f, fl in zip(fr, flips)]))
    monkeypatch.setattr(DK, "encode_targets", encode)
    monkeypatch.setattr(DK, "preprocess_images", frames)
    cases = [R.golden_right_sample(n) for n in R.NAMES_R]
    root = R.make_kitti_dir(tmp_path / "kitti", [(l, w, h) for l, w, h, _, _ in cases], right_seed_of=lambda i: cases[i][4])
    N = len(cases)
    ds = KITTIDataset(R.right_cfg(), root, is_train=True, device="cpu")
    assert len(ds) == int(R.GOLD_R["len"])
    raws = {}
    for i, (n, (lines, w, h, flip, _)) in enumerate(zip(R.NAMES_R, cases)):
        ds.flip_p = 1.0 if flip else 0.0
        raws[n] = ds.load_raw(N + i)
        assert raws[n].flip == flip and raws[n].right
        if n in R.RAISED:
            with pytest.raises(ValueError):
                ds.encode_batch([raws[n]])
            continue
        images, (t,), (idx,), _ = ds.encode_batch([raws[n]])
        assert idx == "%06d" % i
        compare_fields({k: t.get_field(k).numpy() for k in R.GOLD_FIELDS}, R.golden_right_fields(n), n)
        np.testing.assert_allclose(t.get_field("calib").P, R.GOLD_R[n + "_P"], rtol=0, atol=1e-12)
        R.assert_frame_is_the_recorded_one(images[0].numpy(), n)
    # a mixed batch: left s00, right s06 (flipped), left s07 (flipped), right s02
    ds.flip_p = 0.0
    left0 = ds.load_raw(0)
    ds.flip_p = 1.0
    left7 = ds.load_raw(7)
    _, targets, ids, fields = ds.encode_batch([left0, raws["s06"], left7, raws["s02"]])
    assert ids == ["000000", "000006", "000007", "000002"]
    compare_fields({k: targets[1].get_field(k).numpy() for k in R.GOLD_FIELDS}, R.golden_right_fields("s06"), "mixed s06")
    compare_fields({k: targets[3].get_field(k).numpy() for k in R.GOLD_FIELDS}, R.golden_right_fields("s02"), "mixed s02")
    for row, n in ((0, "s00"), (2, "s07")):
        compare_fields({k: targets[row].get_field(k).numpy() for k in LEFT_FIELDS}, {k: GOLD[n + "_" + k] for k in LEFT_FIELDS}, "mixed " + n)
        np.testing.assert_allclose(fields["P"][row].numpy(), GOLD[n + "_P"], rtol=0, atol=1e-12)
