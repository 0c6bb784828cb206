"""CPU checks of the evaluation on the device (TEST.EVAL_ON_DEVICE): the record rule of monoflex_amd/csrc/kitti_eval_pack_math.h,
compiled for the host by the test-only tests/shim/kitti_eval_pack_host.cpp, against numpy's float32 round(4) and against the real
result-file round trip, bit for bit; the LabelTable against read_label_folder; and the refusals, which are all raised on the host."""
import numpy as np
import pytest
import torch

from monoflex_amd import synthetic as S
from monoflex_amd.data import evaluation as EV
from tests.eval_on_device_common import build_pack_shim, same_bits, text_records, write_label_dir


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_pack_shim(tmp_path_factory.mktemp("shim"))


def shim_round4(shim, values):
    values = np.ascontiguousarray(values, dtype=np.float32)
    out = np.full(values.shape, 77.0, dtype=np.float64)
    shim.shim_kitti_pack_round4(values.ctypes.data, values.size, out.ctypes.data)
    return out


def shim_records(shim, rows):
    rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, 14)
    out = np.full((len(rows), 16), 77.0, dtype=np.float64)
    shim.shim_kitti_pack_records(rows.ctypes.data, len(rows), out.ctypes.data)
    return out


def rule_inputs():
    """More than 10^6 float32 values: scores, pixel and metre magnitudes up to 1e4, the special values, denormals, ties of the fourth
    decimal and their negatives, and random finite bit patterns."""
    rs = np.random.RandomState(0)
    n = np.arange(0, 200000, dtype=np.float64)
    ties = ((n + 0.5) / 1e4).astype(np.float32)
    big = np.arange(0, 100000, dtype=np.float64) * 997 % 1e8                             # ties up to 1e4
    big_ties = ((big + 0.5) / 1e4).astype(np.float32)
    denormal = np.concatenate([np.arange(1, 20001, dtype=np.uint32), rs.randint(1, 1 << 23, 20000).astype(np.uint32)]).view(np.float32)
    bits = rs.randint(0, 1 << 32, 200000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    parts = [rs.uniform(0, 1, 200000), rs.uniform(-1e4, 1e4, 200000), rs.uniform(-100, 100, 100000), 10.0 ** rs.uniform(-8, 4, 100000),
             -(10.0 ** rs.uniform(-8, 4, 50000)), [-10.0, -0.0, 0.0, 1.0, -1.0, 1e4, -1e4, 0.00005, -0.00005, 0.99995],
             ties, -ties, big_ties, -big_ties, denormal, -denormal, bits[np.isfinite(bits)]]
    return np.concatenate([np.asarray(p, dtype=np.float32) for p in parts])


def test_record_rule_is_numpy_round4_widened(shim):
    v = rule_inputs()
    assert v.size >= 10 ** 6 and (np.abs(v[v != 0]) < 1.2e-38).sum() > 10000
    with np.errstate(over="ignore", invalid="ignore"):
        want = v.round(4).astype(np.float64)
    got = shim_round4(shim, v)
    diff = got.view(np.uint64) != want.view(np.uint64)
    assert not diff.any(), (int(diff.sum()), v[diff][:5], got[diff][:5], want[diff][:5])
    assert np.signbit(shim_round4(shim, [-0.0]))[0] and shim_round4(shim, [-10.0])[0] == -10.0


def test_record_rule_is_the_text_round_trip(shim, tmp_path):
    """parse_label_text of generate_kitti_3d_detection's file == pack_record, on synthetic detections (and an empty image)."""
    total = 0
    for i in range(12):
        labels = S.synthetic_kitti_labels(3000 + i, 1242, 375, 4 + i % 12, z_range=(5, 38), occl_max=1)
        rows = S.synthetic_detections(3500 + i, labels, 1242, 375, recall=0.9)
        want = text_records(rows, tmp_path / ("%06d.txt" % i))
        got = shim_records(shim, rows)
        assert same_bits(got, want), i
        assert set(got[:, 0]) <= {0.0, 1.0, 2.0} and not got[:, 1:3].any()
        assert np.array_equal(got[:, 8:11], rows[:, [8, 6, 7]].round(4).astype(np.float64))     # l, h, w from h, w, l
        total += len(rows)
    assert total > 50
    assert text_records(np.zeros((0, 14)), tmp_path / "empty.txt").shape == (0, 16) and shim_records(shim, np.zeros((0, 14))).shape == (0, 16)
    odd = np.array([[2, -10.0, -0.0, 0.00005, 1241.99995, 374.5, 1e-42, 1.23456789, 9999.99995, -0.00015, 3e-5, 80.00005, -3.14159265, 1.0]], np.float32)
    assert same_bits(shim_records(shim, odd), text_records(odd, tmp_path / "odd.txt"))


def test_label_table_is_the_label_folder(tmp_path):
    sets = [S.synthetic_kitti_labels(3000 + i, 1242, 375, 3 + i, z_range=(5, 38), occl_max=1) for i in range(5)] + [[]]
    ids = [7, 3, 12, 0, 5, 9]                                       # split-file order is not the sorted order
    label_dir, split = write_label_dir(tmp_path, sets, ids)
    table = EV.LabelTable(label_dir, split)
    want = EV.read_label_folder(label_dir, ids)
    assert len(table) == 6 and table.ids == ids
    assert same_bits(table.gt, np.concatenate(want)) and table.gt.shape[1] == 16
    assert table.gt_off.dtype == np.int32 and np.array_equal(table.gt_off, np.concatenate([[0], np.cumsum([len(w) for w in want])]))
    # the result folder is read back sorted and paired by position: an image's row is the rank of its id
    assert [table.row_of(i) for i in ids] == [3, 1, 5, 0, 2, 4] and table.row_of("000012") == 5
    with pytest.raises(ValueError):
        table.row_of(4)

    class Dataset:
        label_dir, imageset_txt, split = None, None, "val"
    ds = Dataset()
    ds.label_dir, ds.imageset_txt = label_dir, split
    assert EV.LabelTable.of(ds) is EV.LabelTable.of(ds)             # built once per dataset


def test_refusals(tmp_path):
    label_dir, split = write_label_dir(tmp_path, [S.synthetic_kitti_labels(3000 + i, 1242, 375, 4) for i in range(3)])
    table = EV.LabelTable(label_dir, split)
    with pytest.raises(ValueError, match="at most 64 detections per image"):                  # pack_eval_inputs' message
        EV.DeviceResults(table, 1, 65, "cpu")
    with pytest.raises(ValueError, match="at most 64 detections per image"):
        EV.pack_detections(torch.zeros(4, dtype=torch.int32), torch.zeros((3, 1, 65, 14)), torch.zeros((3, 1, 65), dtype=torch.int32))
    with pytest.raises(RuntimeError):                                                         # no CPU fallback
        EV.pack_detections(torch.zeros(4, dtype=torch.int32), torch.zeros((3, 1, 64, 14)), torch.zeros((3, 1, 64), dtype=torch.int32))

    # an image of the split that the pass never delivered: the ValueError of the file path's count mismatch, before any launch
    results = EV.DeviceResults(table, 1, 50, "cpu")
    results.scatter(["000000", "000002"], torch.zeros((2, 50, 14)), torch.ones((2, 50), dtype=torch.int32))
    assert results.seen.tolist() == [True, False, True] and int(results.valid.sum()) == 100
    with pytest.raises(ValueError, match="one detection record array per ground-truth image"):
        results.evaluate(("Car",), ("R40",))
    with pytest.raises(ValueError, match="one detection record array per ground-truth image"):
        EV.pack_eval_inputs(EV.read_label_folder(label_dir, [0, 1, 2]), [np.zeros((0, 16))] * 2, [0], np.zeros((1, 3, 1)))
    with pytest.raises(ValueError):                                                           # an image that is not in the split
        results.scatter(["000004"], torch.zeros((1, 50, 14)), torch.zeros((1, 50), dtype=torch.int32))
    results.scatter(["000001"], torch.zeros((1, 50, 14)), torch.zeros((1, 50), dtype=torch.int32))
    results.check_complete()

    TestSplit = type("TestSplit", (), dict(split="test", label_dir=label_dir, imageset_txt=split, classes=("Car",)))

    class Loader:
        dataset = TestSplit()
    from monoflex_amd.engine.inference import inference, inference_all_depths

    class Model:
        class heads:
            class post_processor:
                output_depth, max_detection = "soft", 50
    with pytest.raises(ValueError, match="test split"):
        EV.LabelTable.of(TestSplit())
    with pytest.raises(ValueError, match="test split"):                                       # at the start of the pass: the loader is never walked
        inference(Model(), Loader(), "kitti_test", device="cpu", output_folder=str(tmp_path / "out"), eval_on_device=True)
    with pytest.raises(ValueError, match="test split"):
        inference_all_depths(Model(), Loader(), "kitti_test", device="cpu", output_folder=str(tmp_path / "out"), eval_on_device=True)
    Loader.dataset = type("Val", (), dict(split="val", label_dir=label_dir, imageset_txt=split, classes=("Car",)))()
    with pytest.raises(ValueError, match="single_pass"):
        inference_all_depths(Model(), Loader(), "kitti_val", device="cpu", output_folder=str(tmp_path / "out"), eval_on_device=True, single_pass=False)
    assert not (tmp_path / "out").exists()


def test_config_key_defaults_off():
    from monoflex_amd.config import get_cfg
    assert get_cfg().TEST.EVAL_ON_DEVICE is False
    assert get_cfg(None, ["TEST.EVAL_ON_DEVICE", "True"]).TEST.EVAL_ON_DEVICE is True


def test_build_and_abi_surface():
    import os
    from monoflex_amd import lib as L
    from monoflex_amd.build import EXTRA_FLAGS, SOURCES
    assert "kitti_eval_pack.hip" in SOURCES and EXTRA_FLAGS["kitti_eval_pack.hip"] == ["-ffp-contract=off"]
    assert "mfx_kitti_eval_pack_count" in L.SYMBOLS and "mfx_kitti_eval_pack_rows" in L.SYMBOLS
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "monoflex_hip.h")).read()
    assert "#define MFX_ABI_VERSION 3 " in header and "mfx_kitti_eval_pack_count(" in header and "mfx_kitti_eval_pack_rows(" in header


def test_loader_mark_switches_the_device_path_on(tmp_path):
    """run_test hands build_test_loader's loaders over without the config: the loader carries TEST.EVAL_ON_DEVICE, and inference() reads it
    (shown by the refusal that only the device path raises, before anything is walked or written)."""
    from monoflex_amd.engine.inference import inference
    label_dir, split = write_label_dir(tmp_path, [[]])
    marked = type("Loader", (), dict(eval_on_device=True, dataset=type("TestSplit", (), dict(split="test", label_dir=label_dir, imageset_txt=split,
                                                                                              classes=("Car",)))()))()
    with pytest.raises(ValueError, match="test split"):
        inference(None, marked, "kitti_test", device="cpu", output_folder=str(tmp_path / "out"))
    assert not (tmp_path / "out").exists()
