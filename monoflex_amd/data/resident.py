"""Resident split (DATALOADER.RESIDENT): decode a split once, keep it on the device, assemble batches from it by index.

`DeviceLoader` decodes every PNG each time it is visited and copies every batch through a fresh pinned buffer.  A KITTI
frame is about 1.4 MB as uint8 and a whole split a few GB, so `ResidentStore.build` walks the dataset once (the same
`RawView` / `load_raw` file reading, with workers), and leaves on the device the raw inputs of the encoder kernels: the
frames HWC back to back in one uint8 arena, their offsets and sizes, the label records, object counts, camera matrices and
view flags.  `ResidentLoader` then draws the flips on the host, sends (index, flip) of a batch up in one small pinned copy
and launches mfx_kitti_preprocess_u8_indexed / mfx_kitti_encode_targets_indexed, which compute slot b from store row
index[b] exactly as the batch entries compute sample b.  It yields what `DeviceLoader` yields.

Not done here: PNG decoding on the device, drawing flips or permutations on the device."""
import ctypes
import logging
import os
import random
import time

import numpy as np
import torch

from .. import lib as L
from ..structures.image_list import ImageList
from . import encode as E
from .collate_batch import RawView, _as_list
from .datasets.kitti_utils import RECORD_WIDTH

STAGING_BYTES = 256 << 20          # upper bound of the pinned memory a build holds: frames are staged, never the split


def plan_rows(dataset, indices):
    """Arena layout from the PNG headers alone (nothing is decoded): (files, img_wh int32[n,2], offsets int64[n], bytes).
    Frames lie HWC back to back, each start 16-byte aligned as in `preprocess_images`. Refuses a frame larger than the input."""
    from PIL import Image
    p, n = dataset.params, len(indices)
    img_wh, offsets, files, total = np.zeros((n, 2), dtype=np.int32), np.zeros(n, dtype=np.int64), [], 0
    for r, idx in enumerate(indices):
        if not 0 <= idx < len(dataset):
            raise IndexError("dataset index %d outside the dataset (%d samples)" % (idx, len(dataset)))
        folder = dataset.image_right_dir if idx >= dataset.num_samples else dataset.image_dir
        path = os.path.join(folder, dataset.image_files[idx % dataset.num_samples])
        with Image.open(path) as im:
            w, h = im.size
        if w > p.in_w or h > p.in_h:
            raise ValueError("%s (%dx%d) is larger than the network input %dx%d" % (path, w, h, p.in_w, p.in_h))
        img_wh[r], offsets[r] = (w, h), total
        total += E._align16(w * h * 3)
        files.append(path)
    return files, img_wh, offsets, total


def walk_rows(dataset, indices, files, img_wh, num_workers, sink):
    """One pass over `indices` through RawView / load_raw (its flip coin is ignored): sink(row, frame) takes each decoded
    frame in row order; returns the host half of the store: records, n_obj, P, right (row r packed as E.pack_inputs packs a
    sample), ids and Calibration objects. Refuses a sample with more objects than MAX_OBJECTS, naming its label file."""
    p, n = dataset.params, len(indices)
    host = dict(records=np.zeros((n, p.max_objs, RECORD_WIDTH), dtype=np.float64), n_obj=np.zeros(n, dtype=np.int32),
                P=np.zeros((n, 3, 4), dtype=np.float64), right=np.zeros(n, dtype=np.int32))
    ids, calibs, r = [], [], 0
    loader = torch.utils.data.DataLoader(RawView(dataset), batch_size=8, sampler=list(indices), num_workers=num_workers, collate_fn=_as_list)
    for batch in loader:
        for s in batch:
            w, h = (int(v) for v in img_wh[r])
            if s.frame.dtype != np.uint8 or s.frame.shape != (h, w, 3):
                raise ValueError("%s: decoded to %s %s, its header says %dx%d" % (files[r], s.frame.shape, s.frame.dtype, w, h))
            if len(s.records) > p.max_objs:
                label = os.path.join(dataset.label_dir, dataset.label_files[indices[r] % dataset.num_samples])
                raise IndexError("%s has %d objects of the detect classes, DATASETS.MAX_OBJECTS is %d" % (label, len(s.records), p.max_objs))
            one = E.pack_inputs([s.records], [s.calib.P], [(w, h)], [0], p)
            host["records"][r], host["n_obj"][r], host["P"][r], host["right"][r] = one["records"][0], one["n_obj"][0], one["P"][0], int(s.right)
            sink(r, s.frame)
            ids.append(s.original_idx)
            calibs.append(s.calib)
            r += 1
    assert r == n
    return host, ids, calibs


class _Staging:
    """Frames -> arena through two pinned halves of `staging_bytes` together (one when the arena fits a half): frames are
    appended in row order at their arena offsets; a full half is sent with one async copy while the other one fills."""

    def __init__(self, arena, total, staging_bytes):
        self.arena, self.half = arena, min(total, staging_bytes // 2)
        self.bufs = [torch.empty(self.half, dtype=torch.uint8, pin_memory=True) for _ in range(1 if total <= self.half else 2)]
        self.events, self.cur, self.base, self.fill = [None] * len(self.bufs), 0, 0, 0

    def add(self, offset, frame):
        if offset + frame.size - self.base > self.half:
            self.flush()
            self.base = offset
        self.bufs[self.cur].numpy()[offset - self.base:offset - self.base + frame.size] = frame.reshape(-1)
        self.fill = offset - self.base + frame.size

    def flush(self):
        if self.fill:
            self.arena[self.base:self.base + self.fill].copy_(self.bufs[self.cur][:self.fill], non_blocking=True)
            self.events[self.cur] = torch.cuda.Event()
            self.events[self.cur].record()
        self.cur, self.fill = (self.cur + 1) % len(self.bufs), 0
        if self.events[self.cur] is not None:
            self.events[self.cur].synchronize()              # the half about to be refilled has left the host


class ResidentStore:
    """Raw inputs of `indices` (dataset indices, row r <-> indices[r]) on the device, host-side ids / sizes / calibrations.
    With every index of the dataset, row i is dataset index i: under DATASETS.USE_RIGHT_IMAGE rows N..2N-1 are the image_3
    frames with P3 and right = 1."""

    def __init__(self, indices, pixels, offsets, img_wh, records, n_obj, P, right, ids, sizes, calibs):
        self.indices = [int(i) for i in indices]
        self._row = {idx: r for r, idx in enumerate(self.indices)}
        self.pixels, self.offsets, self.img_wh, self.records, self.n_obj, self.P, self.right = pixels, offsets, img_wh, records, n_obj, P, right
        self.ids, self.sizes, self.calibs = list(ids), [tuple(int(v) for v in s) for s in sizes], list(calibs)

    def __len__(self):
        return len(self.indices)

    @property
    def nbytes(self):
        return int(self.pixels.numel())

    def row_of(self, idx):
        try:
            return self._row[int(idx)]
        except KeyError:
            raise KeyError("dataset index %d is not in the resident store (%d rows)" % (int(idx), len(self))) from None

    @classmethod
    def build(cls, dataset, indices=None, num_workers=0, max_bytes=None, staging_bytes=STAGING_BYTES):
        device = torch.device(dataset.device)
        if device.type != "cuda":
            raise RuntimeError("a resident store lives on the GPU; there is no CPU fallback")
        t0 = time.perf_counter()
        indices = list(range(len(dataset))) if indices is None else [int(i) for i in indices]
        if not indices:
            raise ValueError("a resident store needs at least one sample")
        files, img_wh, offsets, total = plan_rows(dataset, indices)
        if max_bytes is not None and total > max_bytes:
            raise ValueError("resident store of %d frames needs %d bytes, above the limit of %d (DATALOADER.RESIDENT_MAX_GB)"
                             % (len(indices), total, max_bytes))
        free = torch.cuda.mem_get_info(device)[0]
        if total > free:
            raise ValueError("resident store of %d frames needs %d bytes, the device has %d free" % (len(indices), total, free))
        staging_bytes = min(int(staging_bytes), STAGING_BYTES)
        largest = int(max(E._align16(int(w) * int(h) * 3) for w, h in img_wh))
        if staging_bytes // 2 < largest:
            raise ValueError("staging buffer of %d bytes cannot hold two frames of %d bytes" % (staging_bytes, largest))
        with torch.cuda.device(device):
            pixels = torch.empty(total, dtype=torch.uint8, device=device)
            staging = _Staging(pixels, total, staging_bytes)
            host, ids, calibs = walk_rows(dataset, indices, files, img_wh, num_workers, lambda r, f: staging.add(int(offsets[r]), f))
            staging.flush()
            dev = {k: torch.from_numpy(a).to(device) for k, a in dict(host, offsets=offsets, img_wh=img_wh).items()}
            torch.cuda.synchronize(device)
        logging.getLogger("monoflex.resident").info("resident store: %d rows, %d bytes of frames, built in %.2f s"
                                                    % (len(indices), total, time.perf_counter() - t0))
        return cls(indices, pixels, dev["offsets"], dev["img_wh"], dev["records"], dev["n_obj"], dev["P"], dev["right"], ids, img_wh, calibs)


class ResidentLoader:
    """Iterable of encoded batches like `DeviceLoader` (same dict, `__len__`, re-iterable, `.dataset`), assembled from a
    `ResidentStore` by index. store=None builds one: over the sampler's indices when the sampler is finite (a rank's
    InferenceSampler shard), over the whole dataset otherwise."""

    def __init__(self, dataset, store=None, batch_size=1, sampler=None, batch_sampler=None, check=True, num_workers=0, max_bytes=None):
        if store is None:
            finite = batch_sampler is None and sampler is not None and hasattr(sampler, "__len__")
            store = ResidentStore.build(dataset, list(sampler) if finite else None, num_workers=num_workers, max_bytes=max_bytes)
        if batch_sampler is None:
            base = sampler if sampler is not None else torch.utils.data.SequentialSampler(range(len(dataset)))
            batch_sampler = torch.utils.data.BatchSampler(base, batch_size, drop_last=False)
        self.dataset, self.store, self.batch_sampler, self.check = dataset, store, batch_sampler, check

    def __len__(self):
        return len(self.batch_sampler)

    def __iter__(self):
        for indices in self.batch_sampler:
            yield self.assemble(indices)

    def assemble(self, indices, flips=None):
        """Dataset indices of one batch -> the dict `DeviceBatchCollator` returns. flips: fixed flip decisions (tests);
        None draws them as `load_raw` does, per sample, in batch order."""
        ds, st = self.dataset, self.store
        rows = [st.row_of(i) for i in indices]                   # KeyError before anything is launched
        if flips is None:
            flips = [bool(ds.flip_p > 0 and random.random() < ds.flip_p) for _ in rows]
        if len(flips) != len(rows) or not rows:
            raise ValueError("a batch needs one flip per index and at least one index")
        images, fields, launch_frames, launch_targets = self.prepare(rows, flips)
        launch_frames()
        launch_targets()
        ids = [st.ids[r] for r in rows]
        if self.check:
            E.check_status(fields["status"], ids)
        sizes = [st.sizes[r] for r in rows]
        targets = ds.make_targets(fields, [st.calibs[r] for r in rows], sizes, flips)
        return dict(images=ImageList(images, [tuple(images.shape[-2:])] * len(rows)), targets=tuple(targets), img_ids=tuple(ids), fields=fields)

    def prepare(self, rows, flips):
        """Store rows and flips of one batch -> (images, fields, launch_frames, launch_targets): (index, flip) uploaded in one
        pinned copy, outputs allocated; each launch function enqueues its entry on the current stream and may be repeated
        (the timing tool does)."""
        ds, st = self.dataset, self.store
        p, device, B, N = ds.params, st.pixels.device, len(rows), len(st)
        lib = L.load()
        up = E._upload(dict(index=np.asarray(rows, dtype=np.int32), flip=np.asarray([int(bool(f)) for f in flips], dtype=np.int32)), device)
        fields = E._alloc_outputs(B, p.dims(), device)
        images = torch.empty((B, 3, p.in_h, p.in_w), dtype=torch.float32, device=device)
        d = L.KittiDesc()
        d.records, d.n_obj, d.P, d.img_wh, d.flip = (t.data_ptr() for t in (st.records, st.n_obj, st.P, st.img_wh, up["flip"]))
        for name, (member, _, _) in E.TARGET_FIELDS.items():
            setattr(d, member, fields[name].data_ptr())
        d.B, d.max_objs, d.in_w, d.in_h, d.down, d.num_classes = B, p.max_objs, p.in_w, p.in_h, p.down, p.num_classes
        d.filter_trunc, d.filter_size, d.edge_ratio = p.filter_trunc, p.filter_size, p.edge_ratio
        cfg = None if p.is_yaml() else p.encode_cfg()
        m3, s3 = (ctypes.c_float * 3)(*ds.pixel_mean), (ctypes.c_float * 3)(*ds.pixel_std)

        def launch_frames():
            with torch.cuda.device(device):
                L.check(lib.mfx_kitti_preprocess_u8_indexed(st.pixels.data_ptr(), st.offsets.data_ptr(), st.img_wh.data_ptr(), up["index"].data_ptr(),
                                                            up["flip"].data_ptr(), images.data_ptr(), B, N, p.in_w, p.in_h, m3, s3, int(p.to_bgr),
                                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "mfx_kitti_preprocess_u8_indexed")

        def launch_targets():
            with torch.cuda.device(device):
                L.check(lib.mfx_kitti_encode_targets_indexed(ctypes.byref(d), up["index"].data_ptr(), N,
                                                             st.right.data_ptr() if ds.use_right_img else None,
                                                             None if cfg is None else ctypes.byref(cfg),
                                                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "mfx_kitti_encode_targets_indexed")
        return images, fields, launch_frames, launch_targets
