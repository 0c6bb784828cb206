"""GPU parity of right-camera samples (mfx_kitti_encode_targets_views through the C ABI, DATASETS.USE_RIGHT_IMAGE through the
dataset and loader) against the reference's right-view goldens and the right-view restatement. Rules of tests/kitti_common.py:
integer / mask / index fields identical, float fields to float32 round-off, P within 1e-12, frames by checksum samples."""
import random

import numpy as np
import pytest
import torch

from monoflex_amd import synthetic as S
from monoflex_amd.data import encode as E
from monoflex_amd.data.datasets import kitti_utils as KU
from oracle import kitti_encode_ref as K
from tests import kitti_right_common as R
from tests.kitti_common import GOLD, NAMES, compare_fields, golden_sample

pytestmark = pytest.mark.gpu


def device_encode(samples, rights, check=True, Ps=None):
    out = E.encode_targets([KU.read_label_records(l, R.CLASSES) for l, _, _, _ in samples], Ps or R.view_matrices(rights, len(samples)),
                           [(w, h) for _, w, h, _ in samples], [f for _, _, _, f in samples], E.EncodeParams(), "cuda", check=check,
                           rights=rights)
    return {k: v.cpu().numpy() for k, v in out.items()}


def test_right_view_targets_match_reference_goldens():
    samples = [R.golden_right_sample(n)[:4] for n in R.NAMES_R]
    out = device_encode(samples, [1] * len(samples), check=False)
    for b, n in enumerate(R.NAMES_R):
        if n in R.RAISED:
            assert out["status"][b] != 0, n
            with pytest.raises(ValueError):                           # the exception the reference's failure becomes
                device_encode([samples[b]], [1])
            continue
        assert out["status"][b] == 0, n
        compare_fields({k: v[b] for k, v in out.items()}, R.golden_right_fields(n), n)
        np.testing.assert_allclose(out["P"][b], R.GOLD_R[n + "_P"], rtol=0, atol=1e-12)
    assert sum(int(out["reg_mask"][b].sum()) for b, n in enumerate(R.NAMES_R) if n in R.KEPT) == 75


def test_mixed_batches_match_the_restatement_on_fuzzed_labels():
    """fuzz_sample(1000 .. 1299), each label set as a left-view and as a right-view row of the same batch. Inputs the restatement
    raises on must flag a status and are skipped; every left-view row and at least half of the right-view rows are compared."""
    samples, rights, refs = R.mixed_fuzz_batch(R.FUZZ_SEEDS)
    compared, objects, per = {0: 0, 1: 0}, 0, 60
    for lo in range(0, len(samples), per):
        out = device_encode(samples[lo:lo + per], rights[lo:lo + per], check=False)
        for b, ref in enumerate(refs[lo:lo + per]):
            if ref is None:
                assert out["status"][b] != 0, lo + b
                continue
            assert out["status"][b] == 0, lo + b
            compare_fields({k: v[b] for k, v in out.items()}, ref, "fuzz%d" % (lo + b))
            compared[rights[lo + b]] += 1
            objects += int(ref["reg_mask"].sum())
    n = len(R.FUZZ_SEEDS)
    print("compared: left %d / %d, right %d / %d, %d kept objects" % (compared[0], n, compared[1], n, objects))
    assert compared[0] == n and 2 * compared[1] >= n, compared
    combos = {(r, f) for (_, _, _, f), r, ref in zip(samples, rights, refs) if ref is not None}
    assert combos == {(0, False), (0, True), (1, False), (1, True)}


def test_left_view_rows_of_a_mixed_batch_are_bit_identical_to_the_plain_entry():
    samples = [golden_sample(n)[:4] for n in NAMES] + [R.golden_right_sample(n)[:4] for n in R.KEPT]
    rights = [0] * len(NAMES) + [1] * len(R.KEPT)
    order = np.random.RandomState(0).permutation(len(samples))
    samples, rights = [samples[i] for i in order], [rights[i] for i in order]
    mixed = device_encode(samples, rights)
    recs = [KU.read_label_records(l, R.CLASSES) for l, _, _, _ in samples]
    plain = E.encode_targets(recs, R.view_matrices(rights, len(samples)), [(w, h) for _, w, h, _ in samples], [f for _, _, _, f in samples],
                             E.EncodeParams(), "cuda", check=False)
    zeros = device_encode(samples, [0] * len(samples), check=False, Ps=R.view_matrices(rights, len(samples)))      # same inputs as `plain`
    left = [b for b, r in enumerate(rights) if not r]
    assert len(left) == len(NAMES)
    for k, v in plain.items():
        v = v.cpu().numpy()
        assert zeros[k].tobytes() == v.tobytes(), k                    # all flags 0 == the plain entry, every row
        if k == "hm":
            continue                                                   # compared per row below
        for b in left:
            assert mixed[k][b].tobytes() == v[b].tobytes(), (k, b)
    hm = plain["hm"].cpu().numpy()
    for b in left:
        assert mixed["hm"][b].tobytes() == hm[b].tobytes(), b
    for b in left:                                                     # and they are still the left-view goldens
        n = NAMES[order[b]]
        compare_fields({k: v[b] for k, v in mixed.items()}, {k: GOLD[n + "_" + k] for k in R.GOLD_FIELDS}, n)


def test_dataset_gives_the_fixture_targets_and_frames(tmp_path):
    from monoflex_amd.data import KITTIDataset
    cases = [R.golden_right_sample(n) for n in R.NAMES_R]
    root = R.make_kitti_dir(tmp_path / "kitti", [(l, w, h) for l, w, h, _, _ in cases], right_seed_of=lambda i: cases[i][4])
    N = len(cases)
    ds = KITTIDataset(R.right_cfg(), root, is_train=True)
    assert len(ds) == int(R.GOLD_R["len"]) == 2 * N
    for i, (n, (lines, w, h, flip, _)) in enumerate(zip(R.NAMES_R, cases)):
        ds.flip_p = 1.0 if flip else 0.0
        if n in R.RAISED:
            with pytest.raises(ValueError):
                ds[N + i]
            continue
        img, t, idx = ds[N + i]
        assert idx == "%06d" % i and img.is_cuda
        compare_fields({k: t.get_field(k).cpu().numpy() for k in R.GOLD_FIELDS}, R.golden_right_fields(n), n)
        np.testing.assert_allclose(t.get_field("calib").P, R.GOLD_R[n + "_P"], rtol=0, atol=1e-12)
        R.assert_frame_is_the_recorded_one(img.cpu().numpy(), n)


def test_loader_pass_covers_every_frame_and_view_and_feeds_a_training_step(tmp_path):
    from monoflex_amd.data import DeviceLoader, KITTIDataset
    from monoflex_amd.model.detector import KeypointDetector
    sizes = [(1242, 375), (1224, 370), (1238, 374)]
    cases = [(S.synthetic_kitti_labels(60 + i, w, h, 9), w, h) for i, (w, h) in enumerate(sizes)]
    root = R.make_kitti_dir(tmp_path / "kitti", cases)
    N = len(cases)
    cfg = R.right_cfg()
    cfg.MODEL.PRETRAIN = False
    ds = KITTIDataset(cfg, root, is_train=True)                         # flip coin live: p = 0.5
    assert len(ds) == 2 * N
    g = torch.Generator(); g.manual_seed(0)
    order = torch.randperm(2 * N, generator=g).tolist()                 # one pass over range(2N), as the training sampler permutes it
    random.seed(1)
    batches = list(DeviceLoader(ds, batch_size=2, sampler=order))
    assert len(batches) == N
    seen, mixed_batch = [], None
    for batch in batches:
        views = []
        for b, name in enumerate(batch["img_ids"]):
            P = batch["fields"]["P"][b].cpu().numpy()
            right = bool(np.isclose(P[1, 3], R.P3[1, 3]))
            assert right or np.isclose(P[1, 3], S.KITTI_P2[1, 3])
            flipped = (P[0, 3] > 0) == right                            # P2[0,3] > 0 > P3[0,3]; the flip negates it
            i = int(name)
            w, h = sizes[i]
            frame = R.frame_pixels(R.right_frame_seed(i) if right else R.left_frame_seed(i), w, h)
            assert np.array_equal(batch["images"].tensors[b].cpu().numpy(), K.transform_image(frame, do_flip=flipped)), (name, right)
            ref = R.right_oracle_fields(cases[i][0], w, h, flipped) if right else K.encode_sample(cases[i][0], S.KITTI_P2, w, h, do_flip=flipped)
            assert ref is not None
            compare_fields({k: batch["targets"][b].get_field(k).cpu().numpy() for k in R.GOLD_FIELDS}, ref, "%s right=%s" % (name, right))
            c = batch["targets"][b].get_field("calib")
            np.testing.assert_allclose(c.P, P, rtol=0, atol=1e-12)
            seen.append((i, right)); views.append(right)
        if len(set(views)) == 2:
            mixed_batch = batch
    assert sorted(seen) == sorted((i, r) for i in range(N) for r in (False, True))
    assert mixed_batch is not None, "this permutation of range(2N) is expected to put a left and a right sample into one batch"
    torch.manual_seed(0)
    model = KeypointDetector(cfg).cuda().train()
    loss_dict, _ = model(mixed_batch["images"], list(mixed_batch["targets"]))
    total = sum(loss_dict.values())
    assert torch.isfinite(total) and float(total.detach()) > 0
    total.backward()
    g = model.backbone.base.base_layer[0].weight.grad
    assert g is not None and torch.isfinite(g).all() and float(g.abs().sum()) > 0
