"""Resident split on the GPU (monoflex_amd/data/resident.py, mfx_kitti_preprocess_u8_indexed / mfx_kitti_encode_targets_indexed):
bit equality with the batch path on the generated five-frame directory of tests/resident_common.py, the loader as a drop-in
for DeviceLoader, one training step and one inference() run from resident batches, and the refusals.  The kernels' guard for a
row outside the store is not exercised here (the Python side refuses such an index first; tests/test_resident_cpu.py checks the
guard's host build)."""
import os

import numpy as np
import pytest
import torch

from monoflex_amd.config import get_cfg
from monoflex_amd.data import DeviceLoader, InferenceSampler, KITTIDataset, ResidentLoader, ResidentStore
from monoflex_amd.data import encode as E
from monoflex_amd.data.datasets.kitti import TARGET_ORDER
from tests import kitti_settings_common as KS
from tests import resident_common as RC
from tests.kitti_right_common import right_cfg

pytestmark = pytest.mark.gpu
ROOT = RC.ROOT
YAML = os.path.join(ROOT, "runs", "monoflex.yaml")
FRAME_BYTES = 1280 * 384 * 3


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """<data dir>/kitti/object/training, the place DatasetCatalog looks in."""
    data_dir = tmp_path_factory.mktemp("resident_data")
    os.makedirs(data_dir / "kitti" / "object")
    return RC.make_tree(data_dir / "kitti" / "object" / "training", right_images=True)


def settings_cfg(setting):
    if setting == "defaults":
        return KS.defaults_cfg()                                   # the encoder switches of config/defaults.py: the _cfg path
    if setting == "right":
        return right_cfg()
    return get_cfg(YAML, ["INPUT.TO_BGR", "True"] if setting == "to_bgr" else [])


def batch_path(ds, index, flips):
    raw = [ds.load_raw(i) for i in index]
    for s, f in zip(raw, flips):
        s.flip = bool(f)
    return ds.encode_batch(raw)


# store build keywords per setting: the default single staging buffer, and two small halves that the frames overflow one by one or in pairs
# (reading with worker processes is covered without a GPU, tests/test_resident_cpu.py)
BUILDS = {"yaml": dict(staging_bytes=2 * FRAME_BYTES + 4096), "defaults": {}, "to_bgr": {}, "right": dict(staging_bytes=5 * FRAME_BYTES)}


@pytest.mark.parametrize("setting", ["yaml", "defaults", "to_bgr", "right"])
def test_batches_equal_the_batch_path_bit_for_bit(tree, setting):
    ds = KITTIDataset(settings_cfg(setting), tree, is_train=True)
    assert ds.params.is_yaml() == (setting != "defaults") and ds.params.to_bgr == (setting == "to_bgr")
    store = ResidentStore.build(ds, **BUILDS[setting])
    N = len(store)
    assert N == len(ds) == (10 if setting == "right" else 5) and store.pixels.dtype == torch.uint8 and store.pixels.is_cuda
    assert store.offsets.dtype == torch.int64 and store.img_wh.dtype == torch.int32 and store.records.shape == (N, 40, 14)
    assert store.records.dtype == torch.float64 and store.P.shape == (N, 3, 4) and store.n_obj.dtype == torch.int32
    assert store.right.tolist() == [0] * 5 + [1] * (N - 5)
    loader = ResidentLoader(ds, store=store)
    lists = [([4, 0, 0, 3], [1, 1, 0, 0]), ([2, 1], [0, 1]), ([N - 1], [1]), ([0], [0])]
    if setting == "right":
        lists += [([9, 0, 5, 5, 3], [0, 1, 1, 0, 1]), ([7, 2], [1, 0])]       # both sides of the view boundary, a right row twice
    for index, flips in lists:
        images, targets, ids, fields = batch_path(ds, index, flips)
        got = loader.assemble(index, flips=flips)
        assert got["img_ids"] == tuple(ids)
        assert torch.equal(got["images"].tensors, images), (index, "images")
        for k in E.TARGET_FIELDS:
            assert got["fields"][k].dtype == fields[k].dtype and torch.equal(got["fields"][k], fields[k]), (index, k)
        assert not got["fields"]["status"].any()
        for b, f in enumerate(flips):
            assert np.array_equal(got["targets"][b].get_field("calib").P, targets[b].get_field("calib").P), (index, b)
    if setting == "yaml":                                            # a subset store: rows in the order given, other indices refused
        sub = ResidentLoader(ds, store=ResidentStore.build(ds, indices=[3, 1]))
        images, _, ids, fields = batch_path(ds, [1, 3], [1, 0])
        got = sub.assemble([1, 3], flips=[1, 0])
        assert got["img_ids"] == tuple(ids) and torch.equal(got["images"].tensors, images) and torch.equal(got["fields"]["hm"], fields["hm"])
        with pytest.raises(KeyError, match="dataset index 0 is not in the resident store"):
            sub.assemble([0])


def same_batch(a, b):
    assert a["img_ids"] == b["img_ids"] and torch.equal(a["images"].tensors, b["images"].tensors)
    assert a["images"].image_sizes == b["images"].image_sizes
    assert all(torch.equal(a["fields"][k], b["fields"][k]) for k in E.TARGET_FIELDS)
    for ta, tb in zip(a["targets"], b["targets"]):
        assert ta.fields() == tb.fields() and np.array_equal(ta.get_field("calib").P, tb.get_field("calib").P)
        for k in ta.fields():
            if k != "calib":
                assert torch.equal(ta.get_field(k), tb.get_field(k)), k
        assert set(TARGET_ORDER) <= set(ta.fields())


def test_the_loader_is_a_drop_in_for_device_loader(tree, monkeypatch):
    ds = KITTIDataset(get_cfg(YAML), tree, is_train=True, augment=False)
    resident, plain = ResidentLoader(ds, batch_size=2), DeviceLoader(ds, batch_size=2)
    assert len(resident) == len(plain) == 3 and resident.dataset is ds and len(resident.store) == 5
    first = list(resident)
    for a, b in zip(first, plain):
        same_batch(a, b)
    assert [len(b["img_ids"]) for b in first] == [2, 2, 1]
    for a, b in zip(resident, first):                               # a second iteration gives the same again
        same_batch(a, b)
    # flips are drawn per sample in batch order, as load_raw draws them
    import random
    aug = KITTIDataset(get_cfg(YAML), tree, is_train=True)
    assert aug.flip_p == 0.5
    random.seed(11)
    drawn = [random.random() < 0.5 for _ in range(4)]
    random.seed(11)
    loader = ResidentLoader(aug, store=resident.store)
    same_batch(loader.assemble([0, 1, 2, 3]), loader.assemble([0, 1, 2, 3], flips=drawn))
    assert True in drawn and False in drawn
    # the construction functions switch on DATALOADER.RESIDENT
    from monoflex_amd.data import build_test_loader, make_data_loader
    monkeypatch.setenv("MONOFLEX_DATA_DIR", os.path.dirname(os.path.dirname(os.path.dirname(tree))))
    on = get_cfg(YAML, ["DATALOADER.RESIDENT", "True", "DATALOADER.NUM_WORKERS", "0", "SOLVER.MAX_ITERATION", "2", "SOLVER.IMS_PER_BATCH", "2",
                        "TEST.IMS_PER_BATCH", "2"])
    train = make_data_loader(on, is_train=True)
    assert isinstance(train, ResidentLoader) and len(train) == 2 and len(train.store) == 5
    assert [len(b["img_ids"]) for b in train] == [2, 2]
    tests = build_test_loader(on)
    assert len(tests) == 1 and isinstance(tests[0], ResidentLoader) and tests[0].store.indices == [0, 1, 2, 3, 4]
    val = KITTIDataset(on, tree, is_train=False)
    for a, b in zip(tests[0], DeviceLoader(val, batch_size=2, sampler=InferenceSampler(len(val)))):
        same_batch(a, b)
    off = get_cfg(YAML, ["DATALOADER.NUM_WORKERS", "0", "SOLVER.MAX_ITERATION", "2"])
    assert isinstance(make_data_loader(off, is_train=True), DeviceLoader) and isinstance(build_test_loader(off)[0], DeviceLoader)


def test_a_resident_batch_drives_a_training_step(tree):
    from monoflex_amd.model.detector import KeypointDetector
    cfg = get_cfg(YAML)
    cfg.MODEL.PRETRAIN = False
    ds = KITTIDataset(cfg, tree, is_train=True, augment=False)
    batch = ResidentLoader(ds, store=ResidentStore.build(ds, indices=[0, 1])).assemble([1, 0], flips=[1, 0])
    torch.manual_seed(0)
    model = KeypointDetector(cfg).cuda().train()
    loss_dict, _ = model(batch["images"], list(batch["targets"]))
    total = sum(loss_dict.values())
    assert torch.isfinite(total) and float(total.detach()) > 0
    total.backward()
    g = model.backbone.base.base_layer[0].weight.grad
    assert g is not None and torch.isfinite(g).all() and float(g.abs().sum()) > 0


def test_inference_writes_the_files_of_the_device_loader_run(tree, tmp_path):
    from monoflex_amd import synthetic as S
    from monoflex_amd.engine.inference import inference
    from monoflex_amd.model.detector import KeypointDetector
    cfg = get_cfg(YAML, ["MODEL.COMPUTE_DTYPE", "bf16"])
    cfg.MODEL.PRETRAIN = False
    ds = KITTIDataset(cfg, tree, is_train=False)
    torch.manual_seed(0)
    model = KeypointDetector(cfg).cuda()
    model.load_state_dict(S.synthetic_state_dict(model.state_dict(), seed=0, cls_bias=-1.0))
    plain = DeviceLoader(ds, batch_size=2, sampler=InferenceSampler(len(ds)))
    resident = ResidentLoader(ds, batch_size=2, sampler=InferenceSampler(len(ds)))
    ref_dicts, ref_text, _ = inference(model, plain, "kitti_val", output_folder=str(tmp_path / "plain"))
    got_dicts, got_text, _ = inference(model, resident, "kitti_val", output_folder=str(tmp_path / "resident"))
    files = sorted(os.listdir(tmp_path / "plain" / "data"))
    assert files == ["%06d.txt" % i for i in range(5)] == sorted(os.listdir(tmp_path / "resident" / "data"))
    for f in files:
        assert (tmp_path / "plain" / "data" / f).read_bytes() == (tmp_path / "resident" / "data" / f).read_bytes(), f
    assert sum(len((tmp_path / "plain" / "data" / f).read_bytes()) for f in files) > 0
    assert got_text == ref_text and len(got_dicts) == len(ref_dicts)
    for a, b in zip(got_dicts, ref_dicts):
        assert a.keys() == b.keys() and all(a[k] == b[k] or (np.isnan(a[k]) and np.isnan(b[k])) for k in a)


def test_refusals(tree, tmp_path):
    from PIL import Image
    cfg = get_cfg(YAML)
    ds = KITTIDataset(cfg, tree, is_train=True, augment=False)
    with pytest.raises(ValueError, match=r"needs \d+ bytes, above the limit of 4000000"):
        ResidentStore.build(ds, max_bytes=4000000)
    with pytest.raises(ValueError, match="staging buffer"):
        ResidentStore.build(ds, staging_bytes=FRAME_BYTES)
    big = RC.make_tree(tmp_path / "big")
    Image.fromarray(np.zeros((384, 1281, 3), np.uint8)).save(os.path.join(big, "image_2", "000003.png"))
    with pytest.raises(ValueError, match=r"000003\.png \(1281x384\) is larger than the network input 1280x384"):
        ResidentStore.build(KITTIDataset(cfg, big, is_train=True))
    bad = RC.make_tree(tmp_path / "bad")                            # a truncated object whose 2D box centre lies outside the image: status 2
    with open(os.path.join(bad, "label_2", "000001.txt"), "w") as f:
        f.write("Car 0.50 0 1.50 -300.00 150.00 -100.00 250.00 1.50 1.60 3.90 -12.00 1.65 8.00 0.10\n")
    bad_ds = KITTIDataset(cfg, bad, is_train=True, augment=False)
    store = ResidentStore.build(bad_ds)
    with pytest.raises(ValueError, match=r"sample 2 of the batch \(id 000001\): truncated object"):
        ResidentLoader(bad_ds, store=store).assemble([0, 2, 1])
    unchecked = ResidentLoader(bad_ds, store=store, check=False).assemble([0, 2, 1])
    assert unchecked["fields"]["status"].tolist() == [0, 0, 2]
