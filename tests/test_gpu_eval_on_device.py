"""GPU checks of the evaluation on the device (TEST.EVAL_ON_DEVICE): the pack kernels (mfx_kitti_eval_pack_count / _rows) against the
host text round trip, exactly; the AP report against the file path's on a 30-image set; and inference() / inference_all_depths() /
run_test with the switch on against the same calls with result files, on a generated five-frame directory."""
import os

import numpy as np
import pytest
import torch

from monoflex_amd import synthetic as S
from monoflex_amd.data import evaluation as EV
from tests.eval_on_device_common import ROOT, make_val_dir, same_bits, text_records, write_label_dir

pytestmark = pytest.mark.gpu
NAMES = ("Car", "Pedestrian", "Cyclist")


# ---- the pack kernels ---------------------------------------------------------------------------------------------------------------------
def random_rows(rs, shape):
    """Decode rows with many digits in every column; class ids 0..2."""
    det = np.zeros(shape + (14,), dtype=np.float32)
    det[..., 0] = rs.randint(0, 3, shape)
    det[..., 1] = rs.uniform(-3.2, 3.2, shape)
    det[..., 2:6] = rs.uniform(0, 1242, shape + (4,))
    det[..., 6:9] = rs.uniform(0.3, 5, shape + (3,))
    det[..., 9:12] = rs.uniform(-40, 80, shape + (3,))
    det[..., 12] = rs.uniform(-3.2, 3.2, shape)
    det[..., 13] = rs.uniform(0, 1, shape)
    return det


def pattern_valid(rs, N, NM, K, empty_first, empty_last):
    """Per (image, method): no valid slot, every slot valid, a scattered set, or a prefix; flags are any non-zero int32."""
    valid = np.zeros((N, NM, K), dtype=np.int32)
    for i in range(N):
        for m in range(NM):
            kind = (i + m + 1) % 4
            if kind == 1:
                valid[i, m] = 1
            elif kind == 2:
                valid[i, m] = (rs.rand(K) < 0.4) * rs.choice([1, 7, -1], K)
            elif kind == 3:
                valid[i, m, :rs.randint(0, K + 1)] = 1
    valid[0, :, 0], valid[N - 1, :, K - 1] = 1, 1
    if empty_first:
        valid[0] = 0
    if empty_last:
        valid[N - 1] = 0
    return valid


PACK_CASES = {                       # N, NM, K, method, first image empty, last image empty, no detection at all, first alpha -10
    "one_slot": (1, 1, 1, 0, False, False, False, False),
    "one_image_none": (1, 1, 1, 0, True, True, True, False),
    "partial_wave": (70, 1, 50, 0, True, True, False, False),
    "full_wave_m0": (70, 3, 64, 0, False, True, False, False),
    "full_wave_m2": (70, 3, 64, 2, True, False, False, False),
    "no_detection": (70, 1, 50, 0, True, True, True, False),
    "no_orientation": (70, 3, 50, 2, True, False, False, True),
    "one_image_full": (1, 1, 64, 0, False, False, False, False),
}


@pytest.mark.parametrize("case", sorted(PACK_CASES))
def test_pack_kernels_equal_the_text_round_trip(case, tmp_path):
    N, NM, K, m, empty_first, empty_last, nothing, no_ori = PACK_CASES[case]
    rs = np.random.RandomState(sorted(PACK_CASES).index(case))
    det = random_rows(rs, (N, NM, K))
    valid = pattern_valid(rs, N, NM, K, empty_first, empty_last)
    if case in ("one_slot", "one_image_full"):
        valid[:] = 1
    if nothing:
        valid[:] = 0
    det[valid == 0] = np.nan                                       # a slot that is no detection is never read into a record
    if no_ori:
        i = int(np.nonzero(valid[:, m].any(axis=1))[0][0])
        det[i, m, int(np.nonzero(valid[i, m])[0][0]), 1] = -10.0
    n_gt = rs.randint(0, 13, N)
    gt_off = np.concatenate([[0], np.cumsum(n_gt)]).astype(np.int32)
    # the host side: one result file per image, parsed back, packed as pr_table packs
    dts = [text_records(det[i, m][valid[i, m] != 0], tmp_path / ("%06d.txt" % i)) for i in range(N)]
    arrays, sz, aos = EV.pack_eval_inputs([np.zeros((n, 16)) for n in n_gt], dts, [0], np.zeros((1, 3, 1)))
    dt, dt_off, pair_off, n_dt, n_pairs, dev_aos = EV.pack_detections(torch.from_numpy(gt_off).cuda(), torch.from_numpy(det).cuda(),
                                                                      torch.from_numpy(valid).cuda(), m)
    assert (n_dt, n_pairs, dev_aos) == (sz["n_dt"], sz["n_pairs"], aos)
    assert dt_off.dtype == torch.int32 and np.array_equal(dt_off.cpu().numpy(), arrays["dt_off"])
    assert pair_off.dtype == torch.int64 and np.array_equal(pair_off.cpu().numpy(), arrays["pair_off"])
    assert same_bits(dt[:n_dt].cpu().numpy(), arrays["dt"])
    assert (n_dt == 0) == nothing and dev_aos == (not nothing and not no_ori)
    if not nothing and N > 1:
        assert (len(dts[0]) == 0) == empty_first and (len(dts[-1]) == 0) == empty_last


def test_pack_entries_refuse_bad_sizes():
    from monoflex_amd import lib as L
    lib = L.load()
    z = torch.zeros(8, dtype=torch.int32, device="cuda")
    assert lib.mfx_kitti_eval_pack_count(z.data_ptr(), 1, 1, 65, 0, z.data_ptr(), z.data_ptr(), z.data_ptr(), None) != 0
    assert lib.mfx_kitti_eval_pack_count(z.data_ptr(), 1, 2, 4, 2, z.data_ptr(), z.data_ptr(), z.data_ptr(), None) != 0
    assert lib.mfx_kitti_eval_pack_rows(None, z.data_ptr(), 1, 1, 4, 0, z.data_ptr(), z.data_ptr(), None) != 0
    with pytest.raises(ValueError, match="at most 64 detections per image"):
        EV.pack_detections(z[:2], torch.zeros((1, 1, 65, 14), device="cuda"), torch.zeros((1, 1, 65), dtype=torch.int32, device="cuda"))


# ---- the same answers as the files ---------------------------------------------------------------------------------------------------------
def second_set():
    """The 30 images of test_gpu_kitti_eval.py::test_second_set_against_the_oracle."""
    labels = [S.synthetic_kitti_labels(3000 + i, 1242, 375, 4 + i % 12, z_range=(5, 38), occl_max=1) for i in range(30)]
    dets = [S.synthetic_detections(3500 + i, l, 1242, 375, recall=0.9) for i, l in enumerate(labels)]
    return labels, dets


def device_buffers(dets, rows, K=50, seed=0):
    """Detections of image j in row rows[j], in scattered slots (order kept) of a poisoned (N,1,K,14) buffer."""
    rs = np.random.RandomState(seed)
    det = np.full((len(dets), 1, K, 14), np.nan, dtype=np.float32)
    valid = np.zeros((len(dets), 1, K), dtype=np.int32)
    for j, d in enumerate(dets):
        slots = np.sort(rs.choice(K, len(d), replace=False))
        det[rows[j], 0, slots], valid[rows[j], 0, slots] = d, 1
    return torch.from_numpy(det).cuda(), torch.from_numpy(valid).cuda()


def assert_same_result(got, want):
    (gtext, gret), (wtext, wret) = got, want
    assert gtext == wtext
    assert sorted(gret) == sorted(wret)
    for k in wret:
        assert abs(float(gret[k]) - float(wret[k])) < 1e-9 or (np.isnan(gret[k]) and np.isnan(wret[k])), k


def test_report_equals_the_file_path(tmp_path, monkeypatch):
    labels, dets = second_set()
    label_dir, split = write_label_dir(tmp_path, labels)
    (tmp_path / "data").mkdir()
    for i, d in enumerate(dets):
        EV.generate_kitti_3d_detection(d, str(tmp_path / "data" / ("%06d.txt" % i)))
    want = [EV.evaluate_python(label_dir, str(tmp_path / "data"), split, NAMES, metric=metric) for metric in ("R40", "R11")]
    calls = []
    launch = EV._launch_pr
    monkeypatch.setattr(EV, "_launch_pr", lambda *a: calls.append(1) or launch(*a))
    table = EV.LabelTable(label_dir, split)
    det, valid = device_buffers(dets, list(range(30)))
    got = EV.results_from_device(table, det, valid, NAMES, ("R40", "R11"))
    assert len(calls) == 1                                         # both metrics from ONE PR table
    for g, w in zip(got, want):
        assert_same_result(g, w)
    assert want[0][0] != want[1][0] and sum(v > 1 for v in want[0][1].values()) > 20 and "aos" in want[0][0]
    # a subset of the classes, and the table reused on the same device
    assert_same_result(EV.results_from_device(table, det, valid, ("Car",), ("R40",))[0],
                       EV.evaluate_python(label_dir, str(tmp_path / "data"), split, ("Car",), metric="R40"))
    assert len(table._dev) == 1


def test_pairing_follows_the_sorted_result_folder(tmp_path):
    """A split file that is not sorted: the file path pairs ground truth j (split order) with the j-th smallest result file, and so does
    the row rule -- the detections of image id go to row rank(id)."""
    labels, dets = second_set()
    ids = [21, 4, 17, 9, 2, 30]
    labels, dets = labels[:6], dets[:6]
    label_dir, split = write_label_dir(tmp_path, labels, ids)
    (tmp_path / "data").mkdir()
    for idx, d in zip(ids, dets):
        EV.generate_kitti_3d_detection(d, str(tmp_path / "data" / ("%06d.txt" % idx)))
    table = EV.LabelTable(label_dir, split)
    results = EV.DeviceResults(table, 1, 50, "cuda")
    det, valid = device_buffers(dets, list(range(6)))
    results.scatter(["%06d" % i for i in ids[:4]], det[:4], valid[:4])
    results.scatter(["%06d" % i for i in ids[4:]], det[4:, 0], valid[4:, 0])
    got = results.evaluate(NAMES, ("R40",))[0]
    assert_same_result(got, EV.evaluate_python(label_dir, str(tmp_path / "data"), split, NAMES, metric="R40"))
    ordered, _ = device_buffers(dets, [table.row_of(i) for i in ids])
    assert same_bits(results.det[results.valid != 0].cpu().numpy(), ordered[results.valid != 0].cpu().numpy())


# ---- the loops ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loop(tmp_path_factory):
    """Five generated frames, batch 2 (a last, smaller batch), bf16, synthetic weights, and what the file path returns for them."""
    from monoflex_amd.config import get_cfg
    from monoflex_amd.data import KITTIDataset
    from monoflex_amd.engine.inference import inference, inference_all_depths
    from monoflex_amd.model.detector import KeypointDetector
    base = tmp_path_factory.mktemp("eval_on_device")
    root = make_val_dir(base / "kitti" / "object" / "training", 5)
    cfg = get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml"), ["MODEL.COMPUTE_DTYPE", "bf16"])
    cfg.MODEL.PRETRAIN = False
    ds = KITTIDataset(cfg, root, is_train=False)
    torch.manual_seed(0)
    model = KeypointDetector(cfg).cuda()
    sd = S.synthetic_state_dict(model.state_dict(), seed=0, cls_bias=-1.0)
    model.load_state_dict(sd)
    files = inference(model, make_loader(ds, "device"), "kitti_val", output_folder=str(base / "files"), metrics=("R40", "R11"))
    depths = inference_all_depths(model, make_loader(ds, "device"), "kitti_val", output_folder=str(base / "files"))
    rows = EV.read_label_folder(str(base / "files" / "data"))
    assert sum(len(r) for r in rows) > 0
    return dict(base=base, ds=ds, model=model, sd=sd, files=files, depths=depths)


def make_loader(ds, kind):
    from monoflex_amd.data import DeviceLoader, InferenceSampler, ResidentLoader
    if kind == "resident":
        return ResidentLoader(ds, batch_size=2, sampler=InferenceSampler(len(ds)))
    return DeviceLoader(ds, batch_size=2, sampler=InferenceSampler(len(ds)))


@pytest.mark.parametrize("kind", ["device", "resident"])
def test_inference_on_device_returns_what_the_files_give(loop, kind):
    from monoflex_amd.engine.inference import inference
    out = loop["base"] / ("out_" + kind)
    ret_dicts, result, dis_ious = inference(loop["model"], make_loader(loop["ds"], kind), "kitti_val", output_folder=str(out), metrics=("R40", "R11"),
                                            eval_on_device=True)
    want_dicts, want_result, want_ious = loop["files"]
    assert len(ret_dicts) == 2 and dis_ious == want_ious
    assert_same_result((result, ret_dicts[1]), (want_result, want_dicts[1]))
    assert_same_result((result, ret_dicts[0]), (result, want_dicts[0]))
    assert not (out / "data").exists() and (loop["base"] / "files" / "data").is_dir()


def test_all_depths_on_device(loop):
    from monoflex_amd.engine.inference import EVAL_DEPTH_METHODS, inference_all_depths
    out = loop["base"] / "out_depths"
    ret = inference_all_depths(loop["model"], make_loader(loop["ds"], "device"), "kitti_val", output_folder=str(out), eval_on_device=True)
    assert loop["model"].heads.post_processor.output_depth == "soft"
    assert tuple(ret) == EVAL_DEPTH_METHODS == tuple(loop["depths"])
    for method in EVAL_DEPTH_METHODS:
        assert_same_result(("", ret[method]), ("", loop["depths"][method]))
    assert not out.exists()
    with pytest.raises(ValueError, match="single_pass"):
        inference_all_depths(loop["model"], make_loader(loop["ds"], "device"), "kitti_val", output_folder=str(out), eval_on_device=True, single_pass=False)
    assert loop["model"].heads.post_processor.output_depth == "soft"


def test_through_the_config(loop, monkeypatch):
    """TEST.EVAL_ON_DEVICE True through run_test: the catalog's kitti_train directory is the generated one."""
    from monoflex_amd.config import get_cfg
    from monoflex_amd.engine.test_net import run_test
    monkeypatch.setenv("MONOFLEX_DATA_DIR", str(loop["base"]))
    cfg = get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml"), ["MODEL.COMPUTE_DTYPE", "bf16", "TEST.EVAL_ON_DEVICE", "True", "TEST.IMS_PER_BATCH", "2",
                                                                "DATALOADER.NUM_WORKERS", "0", "OUTPUT_DIR", str(loop["base"] / "out_cfg")])
    cfg.TEST.METRIC = ["R40", "R11"]
    assert cfg.DATASETS.TEST == ("kitti_train",) and cfg.DATASETS.TEST_SPLIT == "val"
    results = run_test(cfg, loop["model"])
    assert len(results) == 1
    ret_dicts, result, _ = results[0]
    assert_same_result((result, ret_dicts[1]), (loop["files"][1], loop["files"][0][1]))
    assert_same_result(("", ret_dicts[0]), ("", loop["files"][0][0]))
    folder = loop["base"] / "out_cfg" / "inference" / "kitti_train"
    assert folder.is_dir() and not (folder / "data").exists()
    cfg.DATASETS.TEST_SPLIT = "test"                                                          # no labels: refused before the pass
    (loop["base"] / "kitti" / "object" / "training" / "ImageSets" / "test.txt").write_text("000000\n")
    with pytest.raises(ValueError, match="test split"):
        run_test(cfg, loop["model"])
