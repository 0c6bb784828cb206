"""Resident split without a GPU: the host half of the store (layout, packing, refusals), the slot -> row mapping of
csrc/kitti_resident_map.h compiled for the host against the batch shim on gathered inputs, the C entries' argument checks and the
configuration keys."""
import ctypes
import os

import numpy as np
import pytest
import torch

from monoflex_amd import lib as L
from monoflex_amd import synthetic as S
from monoflex_amd.data import encode as E
from monoflex_amd.data import resident as R
from monoflex_amd.data.datasets import kitti_utils as KU
from monoflex_amd.data.datasets.kitti import KITTIDataset
from tests import kitti_settings_common as KS
from tests import resident_common as RC
from tests.kitti_right_common import P3, frame_pixels, left_frame_seed, right_cfg, right_frame_seed

ROOT = RC.ROOT
CLASSES = ("Car", "Pedestrian", "Cyclist")
SETTINGS = {"yaml": E.EncodeParams(), "defaults": KS.params_of("defaults")}
INDEX_LISTS = [[4, 0, 0, 3], [2, 1], [4], [0], [4, 3, 2, 1, 0]]         # a repeat, reversed order, the last row, the first row


def flips_of(index):
    """Alternating flips, so that the two copies of a repeated row differ."""
    return [b % 2 == 0 for b in range(len(index))]


@pytest.fixture(scope="module")
def shims(tmp_path_factory):
    d = tmp_path_factory.mktemp("resident_shims")
    return KS.build_cfg_shim(d), RC.build_resident_shim(d)


@pytest.fixture(scope="module")
def rows():
    """Raw inputs of the ten store rows of the fixture under USE_RIGHT_IMAGE: five left views, then their right views."""
    cases = RC.fixture_cases()
    recs = [KU.read_label_records(lines, CLASSES) for lines, _, _ in cases] * 2
    sizes = [(w, h) for _, w, h in cases] * 2
    return recs, [S.KITTI_P2] * 5 + [P3] * 5, sizes, [0] * 5 + [1] * 5


def test_fixture_samples_encode_cleanly(shims, rows):
    """What the GPU tests rely on: every fixture sample has status 0 flipped and unflipped, in both views, under both settings."""
    recs, Ps, sizes, rights = rows
    for name, p in SETTINGS.items():
        for flip in (0, 1):
            out = KS.shim_encode_records(shims[0], recs, Ps, sizes, [flip] * 10, p, rights=rights)
            assert not out["status"].any(), (name, flip, out["status"])
            kept = out["reg_mask"].reshape(10, -1).sum(axis=1)
            assert (kept[[0, 1, 2, 3, 5, 6, 7, 8]] > 0).all() and kept[4] == 0 and kept[9] == 0   # objects are kept; the tiny frame has none


@pytest.mark.parametrize("setting", sorted(SETTINGS))
@pytest.mark.parametrize("views", ["left", "both"])
def test_indexed_mapping_equals_the_batch_shim_on_gathered_inputs(shims, rows, setting, views):
    recs, Ps, sizes, rights = rows
    N = 5 if views == "left" else 10
    p = SETTINGS[setting]
    store = E.pack_inputs(recs[:N], Ps[:N], sizes[:N], [0] * N, p)
    lists = INDEX_LISTS if views == "left" else [[9, 0, 5, 5, 3], [7, 2], [N - 1], [0]]      # both sides of the view boundary
    for index in lists:
        flips = flips_of(index)
        gathered = KS.shim_encode_records(shims[0], [recs[i] for i in index], [Ps[i] for i in index], [sizes[i] for i in index], flips, p,
                                          rights=None if views == "left" else [rights[i] for i in index])
        got = RC.shim_encode_indexed(shims[1], store, index, flips, p, rights=None if views == "left" else rights[:N])
        for k in E.TARGET_FIELDS:
            assert not (got[k] == 77).all(), (index, k)
            assert np.array_equal(got[k], gathered[k]), (setting, views, index, k)
    # cfg == NULL is the yaml setting
    if setting == "yaml":
        got = RC.shim_encode_indexed(shims[1], store, [1, 1], [0, 1], p, cfg=None)
        ref = RC.shim_encode_indexed(shims[1], store, [1, 1], [0, 1], p)
        assert all(np.array_equal(got[k], ref[k]) for k in E.TARGET_FIELDS)


@pytest.mark.parametrize("to_bgr", [False, True])
def test_indexed_frames_equal_the_batch_shim_on_gathered_frames(shims, to_bgr):
    frames = [frame_pixels(left_frame_seed(i), w, h) for i, (w, h) in enumerate(RC.SIZES)]
    offsets, total = np.zeros(5, dtype=np.int64), 0
    for i, f in enumerate(frames):
        offsets[i], total = total, total + E._align16(f.size)
    pixels = np.full(total, 201, dtype=np.uint8)
    for o, f in zip(offsets, frames):
        pixels[o:o + f.size] = f.reshape(-1)
    wh = np.array(RC.SIZES, dtype=np.int32)
    for index in INDEX_LISTS[:3]:
        flips = flips_of(index)
        got = RC.shim_frames_indexed(shims[1], pixels, offsets, wh, index, flips, to_bgr, 1280, 384, KS.K.PIXEL_MEAN, KS.K.PIXEL_STD)
        ref = KS.shim_frames(shims[0], [frames[i] for i in index], flips, to_bgr)
        assert np.array_equal(got, ref), index


def test_a_row_outside_the_store_is_flagged_not_read(shims, rows):
    """Host build of the guard only (the kernels share it through kitti_resident_map.h): status 16, every other output zero, and
    the good slot beside it untouched."""
    recs, Ps, sizes, _ = rows
    p = SETTINGS["yaml"]
    store = E.pack_inputs(recs[:5], Ps[:5], sizes[:5], [0] * 5, p)
    got = RC.shim_encode_indexed(shims[1], store, [5, 2, -1], [1, 1, 0], p)
    ref = RC.shim_encode_indexed(shims[1], store, [2], [1], p)
    assert got["status"].tolist() == [16, 0, 16]
    for k in E.TARGET_FIELDS:
        assert np.array_equal(got[k][1], ref[k][0]), k
        if k != "status":
            assert not got[k][0].any() and not got[k][2].any(), k
    wh = np.array(RC.SIZES, dtype=np.int32)
    img = RC.shim_frames_indexed(shims[1], np.full(2048, 9, np.uint8), np.zeros(5, np.int64), wh, [4, 5, -7], [0, 0, 1], False, 64, 32,
                                 KS.K.PIXEL_MEAN, KS.K.PIXEL_STD)
    assert not img[1].any() and not img[2].any() and img[0].any() and not (img == 77).any()
    assert 16 in E.STATUS_MESSAGES


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    return RC.make_tree(tmp_path_factory.mktemp("resident_tree") / "kitti", right_images=True)


def host_store(ds, indices, num_workers=0):
    files, img_wh, offsets, total = R.plan_rows(ds, indices)
    arena = np.full(total, 201, dtype=np.uint8)

    def sink(r, frame):
        arena[offsets[r]:offsets[r] + frame.size] = frame.reshape(-1)
    host, ids, calibs = R.walk_rows(ds, indices, files, img_wh, num_workers, sink)
    return dict(host, img_wh=img_wh, offsets=offsets, total=total, arena=arena, ids=ids, calibs=calibs)


def test_store_rows_are_the_packed_samples(tree):
    ds = KITTIDataset(right_cfg(), tree, is_train=True)
    assert len(ds) == 10
    h = host_store(ds, list(range(10)))
    raw = [ds.load_raw(i) for i in range(10)]
    ref = E.pack_inputs([s.records for s in raw], [s.calib.P for s in raw], [(s.frame.shape[1], s.frame.shape[0]) for s in raw], [0] * 10, ds.params)
    for k in ("records", "n_obj", "P", "img_wh"):
        assert np.array_equal(h[k], ref[k]) and h[k].dtype == ref[k].dtype, k
    assert h["n_obj"][:4].min() >= 5 and h["n_obj"][4] == 0
    # frames back to back, in order, each start 16-byte aligned, gaps shorter than 16 bytes
    sizes = [s.frame.size for s in raw]
    assert not (h["offsets"] % 16).any() and h["offsets"][0] == 0
    for i in range(9):
        assert 0 <= h["offsets"][i + 1] - (h["offsets"][i] + sizes[i]) < 16, i
    assert h["total"] == h["offsets"][9] + E._align16(sizes[9])
    for i, s in enumerate(raw):
        assert np.array_equal(h["arena"][h["offsets"][i]:h["offsets"][i] + sizes[i]], s.frame.reshape(-1)), i
    # rows N..2N-1: the image_3 frames with P3 and right = 1
    assert h["right"].tolist() == [0] * 5 + [1] * 5
    assert all(np.array_equal(h["P"][i], S.KITTI_P2) for i in range(5)) and all(np.array_equal(h["P"][i], P3) for i in range(5, 10))
    assert np.array_equal(h["arena"][h["offsets"][7]:h["offsets"][7] + sizes[7]], frame_pixels(right_frame_seed(2), 1241, 376).reshape(-1))
    assert h["ids"] == ["%06d" % (i % 5) for i in range(10)] and np.array_equal(h["calibs"][6].P, P3)
    # a subset store keeps the order it was given, also when worker processes read the files
    sub = host_store(ds, [8, 1], num_workers=2)
    assert sub["ids"] == ["000003", "000001"] and sub["right"].tolist() == [1, 0] and np.array_equal(sub["records"][1], ref["records"][1])


def test_build_time_refusals_on_the_host(tree, tmp_path):
    from PIL import Image
    from monoflex_amd.config import get_cfg
    cfg = get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml"))
    ds = KITTIDataset(cfg, tree, is_train=True)
    with pytest.raises(IndexError, match="7"):
        R.plan_rows(ds, [0, 7])
    big = RC.make_tree(tmp_path / "big")
    Image.fromarray(np.zeros((385, 1280, 3), np.uint8)).save(os.path.join(big, "image_2", "000002.png"))
    with pytest.raises(ValueError, match=r"000002\.png \(1280x385\) is larger than the network input 1280x384"):
        R.plan_rows(KITTIDataset(cfg, big, is_train=True), list(range(5)))
    crowded = KITTIDataset(get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml"), ["DATASETS.MAX_OBJECTS", "3"]), tree, is_train=True)
    with pytest.raises(IndexError, match=r"000000\.txt has \d+ objects of the detect classes, DATASETS.MAX_OBJECTS is 3"):
        host_store(crowded, [4, 0])


def test_lookups_outside_the_store_are_refused_before_any_library_call(tree, monkeypatch):
    from monoflex_amd.config import get_cfg
    ds = KITTIDataset(get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml")), tree, is_train=False)
    h = host_store(ds, [3, 1])
    t = {k: torch.from_numpy(h[k]) for k in ("arena", "offsets", "img_wh", "records", "n_obj", "P", "right")}
    store = R.ResidentStore([3, 1], t["arena"], t["offsets"], t["img_wh"], t["records"], t["n_obj"], t["P"], t["right"], h["ids"], h["img_wh"],
                            h["calibs"])
    assert len(store) == 2 and store.row_of(3) == 0 and store.row_of(1) == 1 and store.nbytes == h["total"]

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", no_library)
    loader = R.ResidentLoader(ds, store=store, batch_size=2, sampler=[3, 1])
    assert len(loader) == 1 and loader.dataset is ds
    for bad in (0, 5, -1, 99):
        with pytest.raises(KeyError, match="dataset index %d is not in the resident store" % bad):
            loader.assemble([3, bad])
    with pytest.raises(RuntimeError, match="GPU"):
        R.ResidentStore.build(KITTIDataset(get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml")), tree, is_train=False, device="cpu"))


def test_entries_refuse_bad_arguments():
    lib, null = L.load(), ctypes.c_void_p(0)
    one = ctypes.c_void_p(16)                                      # any non-null value: the checks fail before anything is read
    m3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    pre = lib.mfx_kitti_preprocess_u8_indexed
    assert pre(None, one, one, one, one, one, 1, 1, 1280, 384, m3, m3, 0, null) != 0 and b"mfx_kitti_preprocess_u8_indexed: null pointer" in lib.mfx_last_error()
    assert pre(one, one, one, None, one, one, 1, 1, 1280, 384, m3, m3, 0, null) != 0 and b"null pointer" in lib.mfx_last_error()
    assert pre(one, one, one, one, one, one, 1, 1, 1280, 384, None, m3, 0, null) != 0 and b"null pointer" in lib.mfx_last_error()
    for B, N in ((0, 1), (-2, 1), (1, 0), (1, -1)):
        assert pre(one, one, one, one, one, one, B, N, 1280, 384, m3, m3, 0, null) != 0 and b"mfx_kitti_preprocess_u8_indexed: bad sizes" in lib.mfx_last_error()
    enc = lib.mfx_kitti_encode_targets_indexed
    assert enc(None, one, 1, None, None, null) != 0 and b"null descriptor" in lib.mfx_last_error()
    d = L.KittiDesc()
    d.B, d.max_objs, d.in_w, d.in_h, d.down, d.num_classes = 1, 40, 1280, 384, 4, 3
    assert enc(ctypes.byref(d), None, 1, None, None, null) != 0 and b"null index" in lib.mfx_last_error()
    for N in (0, -3):
        assert enc(ctypes.byref(d), one, N, None, None, null) != 0 and b"mfx_kitti_encode_targets_indexed: bad sizes" in lib.mfx_last_error()
    d.B = 0
    assert enc(ctypes.byref(d), one, 5, None, None, null) != 0 and b"bad sizes" in lib.mfx_last_error()
    d.B = 1
    assert enc(ctypes.byref(d), one, 5, None, None, null) != 0 and b"pointer of the descriptor" in lib.mfx_last_error()


def test_the_switch_is_off_by_default():
    from monoflex_amd.config import get_cfg
    cfg = get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml"))
    assert cfg.DATALOADER.RESIDENT is False and cfg.DATALOADER.RESIDENT_MAX_GB == 64
    on = get_cfg(os.path.join(ROOT, "runs", "monoflex.yaml"), ["DATALOADER.RESIDENT", "True", "DATALOADER.RESIDENT_MAX_GB", "0.5"])
    assert on.DATALOADER.RESIDENT is True and on.DATALOADER.RESIDENT_MAX_GB == 0.5
    from monoflex_amd.build import EXTRA_FLAGS, SOURCES
    assert "kitti_resident.hip" in SOURCES and EXTRA_FLAGS["kitti_resident.hip"] == ["-ffp-contract=off"]
