"""DeviceImage: an RGB u8 image resident in HBM with the PIL methods the zoom chain calls.

replaces: the `PIL.Image` objects handled by cut_image / resize_image in the reference
(/root/reference/src/eval/infer.py:41-85,215,237): `.size`, `.width`, `.height`, `.crop(box)` (zero fill outside),
`.resize((w, h), Image.BICUBIC)`, `.convert("RGB")`.  crop() is lazy (a box on the parent tile); resize() runs ONE
fused crop+bicubic launch of the HIP front-end on the full-resolution tile, so a 5000-px tile is uploaded once
and every view / zoom of every question about it reads it in place.
"""
from __future__ import annotations

import itertools

import numpy as np
import torch

from . import _lib

BICUBIC = 3
_ids = itertools.count(1)


class DeviceImage:
    def __init__(self, base: torch.Tensor, engine, box=None, key=None):
        assert base.dtype == torch.uint8 and base.dim() == 3 and base.shape[2] == 3 and base.is_cuda
        self.base = base.contiguous()
        self.engine = engine
        h, w = int(base.shape[0]), int(base.shape[1])
        self.box = tuple(int(v) for v in box) if box is not None else (0, 0, w, h)
        # identity used by the processor / model to reuse ViT features and prompt KV across the two stages
        self.key = key if key is not None else ("img", next(_ids))

    # ---- constructors
    @classmethod
    def from_numpy(cls, arr: np.ndarray, engine):
        arr = np.ascontiguousarray(arr, dtype=np.uint8)
        if arr.ndim != 3 or arr.shape[2] != 3:
            raise ValueError("expected an [H, W, 3] uint8 array")
        return cls(torch.from_numpy(arr).to(engine.device, non_blocking=False), engine)

    @classmethod
    def from_pil(cls, img, engine):
        return cls.from_numpy(np.asarray(img.convert("RGB")), engine)

    @classmethod
    def open(cls, path: str, engine, device_decode: bool = False):
        """device_decode: an LZW / PackBits TIFF (tiff_plan) travels compressed and is decoded by the engine (Engine.upload_tiff);
        every other file, and a file with a defective chunk, is decoded on the host as without the option."""
        from PIL import Image

        if device_decode:
            plan = tiff_plan(path)
            if plan is not None:
                try:
                    return cls(engine.upload_tiff(plan), engine)
                except ValueError:   # a defective or old-style chunk (TiffChunkError): the host decodes the file, or raises as it always did
                    pass
                except _lib.ZoomEarthError as ex:
                    if ex.code not in (_lib.ZE_ERR_INVALID, _lib.ZE_ERR_NOMEM):   # a shape the library refuses, no room for the staging
                        raise
        Image.MAX_IMAGE_PIXELS = None  # 5000-px tiles (src/eval/infer.py:18)
        with Image.open(path) as im:
            return cls.from_pil(im, engine)

    # ---- PIL surface
    @property
    def width(self) -> int:
        return self.box[2] - self.box[0]

    @property
    def height(self) -> int:
        return self.box[3] - self.box[1]

    @property
    def size(self):
        return (self.width, self.height)

    def convert(self, mode: str):
        if mode != "RGB":
            raise ValueError("DeviceImage is RGB only")
        return self

    def crop(self, box):
        x0, y0, x1, y1 = (int(v) for v in box)
        bx, by = self.box[0], self.box[1]
        return DeviceImage(self.base, self.engine, (bx + x0, by + y0, bx + x1, by + y1),
                           key=("crop", self.key, (x0, y0, x1, y1)))

    def resize(self, size, resample=BICUBIC, **kw):
        if resample != BICUBIC:
            raise ValueError("only Image.BICUBIC is implemented on the device")
        w, h = int(size[0]), int(size[1])
        out = self.engine.crop_resize(self.base, self.box, (w, h))
        return DeviceImage(out, self.engine, key=("resize", self.key, (w, h)))

    def tensor(self) -> torch.Tensor:
        """Materialised u8 [H, W, 3] device tensor of this view (crop applied, zero fill outside the tile)."""
        h, w = int(self.base.shape[0]), int(self.base.shape[1])
        if self.box == (0, 0, w, h):
            return self.base
        return self.engine.crop_resize(self.base, self.box, (self.width, self.height))

    def numpy(self) -> np.ndarray:
        return self.tensor().cpu().numpy()


def decode_rgb(path: str) -> np.ndarray:
    """Host decode of a tile file to RGB u8 [H, W, 3] (Image.open(fp).convert("RGB"), src/eval/infer.py:215,237)."""
    from PIL import Image

    Image.MAX_IMAGE_PIXELS = None
    with Image.open(path) as im:
        raw = _raw_rgb_strips(im)
        if raw is None:
            return np.array(im.convert("RGB"), dtype=np.uint8)  # a writable, contiguous copy
        w, h = im.size
    # Uncompressed 8-bit RGB (the usual way a 5000-px TIFF tile is stored): the file's strips ARE the pixels.  Reading them
    # straight into the array keeps the interpreter lock free (readinto releases it) -- through PIL the same tile goes
    # through load() + tobytes(), 64 KB at a time under the lock, and three decode threads then take 0.66 s per tile instead of
    # 0.16 and starve the threads that drive the GPU (measured on the real entry point: tools/bench_infer_e2e.py)
    arr = np.empty((h, w, 3), dtype=np.uint8)
    with open(path, "rb", buffering=0) as f:
        for y0, y1, off in raw:
            f.seek(off)
            mv = memoryview(arr[y0:y1]).cast("B")
            got = 0
            while got < len(mv):
                n = f.readinto(mv[got:])
                if not n:
                    raise OSError(f"{path}: truncated image data")
                got += n
    return arr


def _raw_rgb_strips(im):
    """[(first row, end row, file offset)] when the opened image is uncompressed, tightly packed, top-down 8-bit RGB stored
    in full-width strips (PIL's tile list says so); None otherwise."""
    try:
        if im.mode != "RGB" or not im.tile:
            return None
        w, h = im.size
        out, y = [], 0
        for t in im.tile:
            name, (x0, y0, x1, y1), off, args = t[0], t[1], t[2], t[3]
            rawmode = args if isinstance(args, str) else args[0]
            stride = 0 if isinstance(args, str) or len(args) < 2 else args[1]
            orient = 1 if isinstance(args, str) or len(args) < 3 else args[2]
            if name != "raw" or rawmode != "RGB" or stride not in (0, 3 * w) or orient != 1 or x0 != 0 or x1 != w or y0 != y:
                return None
            out.append((y0, y1, int(off)))
            y = y1
        return out if y == h else None
    except Exception:
        return None


# ---------------------------------------------------------------------------------------------------------------- TIFF decode plan
TIFF_LZW, TIFF_PACKBITS = 5, 32773
TIFF_MAX_CHUNK_BYTES = 1 << 20   # what one chunk may store (ZT_MAX_CHUNK_OUT of csrc/ze_tiff_codec.h: 20 bits of offset in the string table)
_TIFF_ALIGN = 16                 # a chunk starts on a 16-byte boundary of the upload buffer (the bit reader fetches 16 aligned bytes)
# tags that say nothing about how the pixels are stored (names, resolution, dates, XMP / ICC / GeoTIFF / GDAL metadata); any tag outside
# this set and the ones tiff_plan reads makes the file one the plan does not understand
_TIFF_INERT_TAGS = frozenset((269, 270, 271, 272, 282, 283, 285, 296, 305, 306, 315, 316, 700, 33432, 33550, 33922, 34264, 34675, 34735, 34736,
                              34737, 42112, 42113))
_TIFF_READ_TAGS = frozenset((254, 256, 257, 258, 259, 262, 266, 273, 274, 277, 278, 279, 284, 317, 322, 323, 324, 325, 339))


class TiffChunkError(ValueError):
    """The device reported a defective chunk (non-zero status words): the tile is decoded on the host instead."""


class TiffPlan:
    """What the device needs to decode one LZW / PackBits RGB TIFF: where every chunk (strip or tile) lies in the file and in the image.

    table: int32 [n_chunks, 8] = {offset in the upload buffer, byte count, x0, y0, w, h of the destination rectangle, stored w,
    stored h} -- the chunk table of ze_tile_upload_tiff; n_bytes: the size of the upload buffer (a multiple of 16); file_offsets: where
    read_into finds each chunk in the file.  Edge tiles are stored padded to chunk_w x chunk_h, as TIFF stores them."""

    def __init__(self, path, width, height, compression, predictor, tiled, chunk_w, chunk_h, file_offsets, table, n_bytes):
        self.path, self.width, self.height = path, int(width), int(height)
        self.compression, self.predictor, self.tiled = int(compression), int(predictor), bool(tiled)
        self.chunk_w, self.chunk_h = int(chunk_w), int(chunk_h)
        self.file_offsets, self.table, self.n_bytes = file_offsets, table, int(n_bytes)

    @property
    def n_chunks(self) -> int:
        return int(self.table.shape[0])

    def read_into(self, buf) -> bool:
        """The compressed chunks into buf (a writable u8 buffer of n_bytes, ideally pinned), each at its table offset; readinto releases
        the interpreter lock.  False when a chunk turns out to be pre-6.0 LZW (LSB-first codes: libtiff knows it by a first byte of 0
        and a set low bit in the second), which the device does not decode."""
        mv = memoryview(buf).cast("B")
        with open(self.path, "rb", buffering=0) as f:
            for off, (o, n) in zip(self.file_offsets.tolist(), self.table[:, :2].tolist()):
                f.seek(off)
                got = 0
                while got < n:
                    k = f.readinto(mv[o + got:o + n])
                    if not k:
                        raise OSError(f"{self.path}: truncated image data")
                    got += k
                if self.compression == TIFF_LZW and n >= 2 and mv[o] == 0 and (mv[o + 1] & 1):
                    return False
        return True


def tiff_plan(path: str):
    """The TiffPlan of an LZW or PackBits 8-bit RGB TIFF, read from its tags through Pillow without decoding a pixel; None for every
    file the device does not decode -- another compression (none included: decode_rgb reads those strips directly), palette / grey /
    RGBA / extra samples, 16-bit, planar 2, FillOrder 2, an orientation, old-style LZW, a chunk that stores more than 1 MiB, any tag the
    plan does not understand, no TIFF at all.  None always means: use decode_rgb as before."""
    try:
        from PIL import Image, TiffImagePlugin

        Image.MAX_IMAGE_PIXELS = None
        with Image.open(path) as im:
            if not isinstance(im, TiffImagePlugin.TiffImageFile) or getattr(im, "n_frames", 1) != 1:
                return None
            tags = dict(im.tag_v2)
            w, h = im.size
        if any(t not in _TIFF_READ_TAGS and t not in _TIFF_INERT_TAGS for t in tags):
            return None

        def one(tag, default):
            v = tags.get(tag, default)
            return v[0] if isinstance(v, tuple) and len(v) == 1 else v

        compression, predictor = one(259, 1), one(317, 1)
        if compression not in (TIFF_LZW, TIFF_PACKBITS) or predictor not in (1, 2):
            return None
        if tuple(tags.get(258, ())) != (8, 8, 8) or one(277, 1) != 3 or one(262, None) != 2 or one(284, 1) != 1:
            return None
        if one(266, 1) != 1 or one(274, 1) != 1 or one(254, 0) != 0 or tuple(tags.get(339, (1, 1, 1))) != (1, 1, 1):
            return None
        if one(256, w) != w or one(257, h) != h or w < 1 or h < 1:
            return None
        has_strips, has_tiles = 273 in tags or 279 in tags, any(t in tags for t in (322, 323, 324, 325))
        if has_strips == has_tiles:
            return None
        if has_tiles:
            tw, th = int(one(322, 0)), int(one(323, 0))
            if tw < 1 or th < 1:
                return None
            across, down = -(-w // tw), -(-h // th)
            offs, counts = tags.get(324), tags.get(325)
            rects = [(x * tw, y * th, min(tw, w - x * tw), min(th, h - y * th), tw, th) for y in range(down) for x in range(across)]
            chunk_w, chunk_h = tw, th
        else:
            rps = min(int(one(278, h)), h)
            if rps < 1:
                return None
            offs, counts = tags.get(273), tags.get(279)
            rects = [(0, y, w, min(rps, h - y), w, min(rps, h - y)) for y in range(0, h, rps)]
            chunk_w, chunk_h = w, rps
        if offs is None or counts is None or len(offs) != len(rects) or len(counts) != len(rects):
            return None
        if chunk_w * chunk_h * 3 > TIFF_MAX_CHUNK_BYTES or min(counts) < 1 or min(offs) < 8 or max(counts) >= 1 << 30:
            return None
        counts = np.asarray(counts, dtype=np.int64)
        starts = np.zeros(len(rects), dtype=np.int64)
        padded = (counts + _TIFF_ALIGN - 1) // _TIFF_ALIGN * _TIFF_ALIGN
        starts[1:] = np.cumsum(padded)[:-1]
        n_bytes = int(padded.sum())
        if n_bytes >= 1 << 31:
            return None
        table = np.empty((len(rects), 8), dtype=np.int32)
        table[:, 0], table[:, 1], table[:, 2:] = starts, counts, np.asarray(rects, dtype=np.int32)
        plan = TiffPlan(path, w, h, compression, predictor, has_tiles, chunk_w, chunk_h, np.asarray(offs, dtype=np.int64), table, n_bytes)
        if compression == TIFF_LZW:   # the old-style header shows in the first two bytes of a chunk: look at the first one now
            with open(path, "rb") as f:
                f.seek(int(offs[0]))
                head = f.read(2)
            if len(head) == 2 and head[0] == 0 and (head[1] & 1):
                return None
        return plan
    except Exception:
        return None


class _Compressed:
    """A tile the worker read but did not decode: its plan and the pooled pinned buffer that holds its chunks."""

    def __init__(self, plan, buf):
        self.plan, self.buf = plan, buf
        self._ze_pool_buffer = buf


class TilePrefetcher:
    """One tile decode per TILE instead of two per QUESTION, and off the GPU's critical path.

    replaces: the two `Image.open(image_fp).convert("RGB")` calls per question of the reference loop
    (/root/reference/src/eval/infer.py:215,237).  A 5000-px TIFF decodes in 0.2-0.5 s on one
    core -- as long as a whole question takes on the GPU -- so the decode of the NEXT distinct tile of the question
    stream runs in a background thread (PIL releases the GIL inside its decoders) into pinned host memory while the
    current tile's questions run; `get(path)` then only pays the PCIe copy.  Questions arrive grouped by tile
    (accel.shard_by_tile), so one tile ahead is enough; one resident tile + one decoded-ahead tile bound the memory.

        pf = TilePrefetcher(paths_in_question_order, engine)
        for q in questions: tile = pf.get(q.path)
    """

    def __init__(self, paths, engine, decode=decode_rgb, pin: bool = True, depth: int = 1, workers: int = 1, device_decode: bool = False):
        """depth: decoded tiles held ahead of the one in use (75 MB of pinned memory each at 5000 px); workers: decode
        threads (a stream that answers 50 questions/s needs ~5 tiles/s: more than one core's worth of TIFF / PNG decode).
        device_decode: a tile that has a tiff_plan (LZW / PackBits RGB TIFF) is only READ by the worker -- its compressed chunks, into a
        pooled pinned buffer -- and get() has the device decode it (ze_tile_upload_tiff); a tile without a plan, or one whose status
        words name a defect, is decoded by `decode` as without the option and counted in `fallbacks`."""
        import threading

        self._engine = engine
        self._decode = decode
        self._pin = pin
        self._depth, self._workers = max(1, int(depth)), max(1, int(workers))
        order = []
        for p in paths:  # distinct tiles in first-use order
            if not order or order[-1] != p:
                order.append(p)
        self._order = order
        self._next = 0            # index in _order of the next tile to decode ahead
        self._ready = {}          # path -> decoded host array / exception
        self._busy = 0            # decodes in progress
        self._current = (None, None)
        self._cv = threading.Condition()
        self._skipped = set()     # tiles the caller will not ask for after all (claimed by another rank: accel.TileClaims)
        self._in_copy = []        # (event, pinned buffer) of uploads that may still be running
        self._pinned = []         # free pinned staging buffers, reused tile after tile (hipHostMalloc of 75 MB per tile costs
        #                           more than the decode itself and serialises with the GPU's work)
        self._device_decode = bool(device_decode)
        self._copy_stream = None
        self.decodes = 0
        self.device_decodes = 0   # tiles the device decoded
        self.fallbacks = 0        # tiles of a device_decode prefetcher that the host decoded after all (no plan, or a defective chunk)
        self.decode_s = 0.0       # seconds spent inside the decoder (all threads)
        self.wait_s = 0.0         # seconds get() waited for a tile that was not ready
        self._kick()

    def _kick(self):
        import threading

        with self._cv:
            while (self._next < len(self._order) and self._busy < self._workers
                   and len(self._ready) + self._busy < self._depth):
                path = self._order[self._next]
                self._next += 1
                if path in self._skipped:
                    continue
                self._busy += 1
                threading.Thread(target=self._work, args=(path,), daemon=True).start()

    def _take_pinned(self, n: int):
        """A pinned buffer of the pool that holds n bytes (allocated on first use, recycled by get() once uploaded)."""
        buf = None
        with self._cv:
            for i, b in enumerate(self._pinned):
                if b.numel() >= n:
                    buf = self._pinned.pop(i)
                    break
        if buf is None:
            buf = torch.empty(n, dtype=torch.uint8).pin_memory()
        return buf

    def _to_pinned(self, arr):
        """The decoded tile in a pinned buffer of the pool."""
        n = int(arr.size)
        buf = self._take_pinned(n)
        view = buf[:n].view(arr.shape)
        view.numpy()[...] = arr
        view._ze_pool_buffer = buf
        return view

    def _read_compressed(self, path):
        """The tile's compressed chunks in a pinned buffer, or None when it has no plan (the host decodes it)."""
        plan = tiff_plan(path)
        if plan is None:
            return None
        buf = self._take_pinned(plan.n_bytes)
        ok = False
        try:
            ok = plan.read_into(buf[:plan.n_bytes].numpy())
        finally:
            if not ok:
                with self._cv:
                    self._pinned.append(buf)
        return _Compressed(plan, buf) if ok else None

    def _host_decode(self, path):
        arr = self._decode(path)
        if self._pin and torch.cuda.is_available():
            arr = self._to_pinned(arr)
        return arr

    def _work(self, path):
        import time
        t0 = time.perf_counter()
        try:
            arr = self._read_compressed(path) if self._device_decode else None
            if arr is None:
                if self._device_decode:
                    with self._cv:
                        self.fallbacks += 1
                arr = self._host_decode(path)
        except Exception as ex:  # surfaced by get()
            arr = ex
        with self._cv:
            if path in self._skipped:     # skipped while it was being decoded: the staging buffer goes back to the pool
                buf = getattr(arr, "_ze_pool_buffer", None)
                if buf is not None:
                    self._pinned.append(buf)
            else:
                self._ready[path] = arr
            self._busy -= 1
            self.decodes += 1
            self.decode_s += time.perf_counter() - t0
            self._cv.notify_all()
        self._kick()

    def skip(self, path: str) -> None:
        """The caller will not get() this tile (work stealing: another rank claimed it): a copy decoded ahead is dropped and its
        place in the look-ahead window goes to the next tile."""
        with self._cv:
            self._skipped.add(path)
            arr = self._ready.pop(path, None)
            buf = getattr(arr, "_ze_pool_buffer", None) if arr is not None else None
            if buf is not None:
                self._pinned.append(buf)
        self._kick()

    def ready(self, path: str) -> bool:
        """True when get(path) would not wait for a decode in progress (the caller has better things to do meanwhile)."""
        if self._current[0] == path:
            return True
        with self._cv:
            return path in self._ready or path not in self._order[:self._next]

    def get(self, path: str) -> DeviceImage:
        if self._current[0] == path:
            return self._current[1]
        import time
        t0 = time.perf_counter()
        with self._cv:
            while path not in self._ready:
                queued = path in self._order[:self._next]     # requested from a worker: in progress or done
                if not queued or (self._busy == 0 and path not in self._ready):
                    break
                self._cv.wait(timeout=0.05)
            arr = self._ready.pop(path, None)
        if arr is None:  # out-of-order request: decode here
            arr = self._read_compressed(path) if self._device_decode else None
            if arr is None:
                self.fallbacks += int(self._device_decode)
                arr = self._decode(path)
            self.decodes += 1
        self.wait_s += time.perf_counter() - t0
        if isinstance(arr, Exception):
            self._kick()
            raise arr
        if isinstance(arr, _Compressed):
            # the compressed chunks go up and the device decodes them; the status words come back where the upload is waited for
            # -- on a copy stream of the prefetcher's own, so that the wait is for this tile alone and not for the chains' queued steps
            if self._copy_stream is None:
                self._copy_stream = torch.cuda.Stream(self._engine.device)
            try:
                with torch.cuda.stream(self._copy_stream):
                    dev, status = self._engine.tile_upload_tiff(arr.plan, arr.buf)
                    bad = bool(status.any().item())   # (waits for the copy and the kernels on the copy stream)
                dev.record_stream(torch.cuda.current_stream(self._engine.device))   # the caller's stream reads it from here on
            except _lib.ZoomEarthError as ex:
                if ex.code not in (_lib.ZE_ERR_INVALID, _lib.ZE_ERR_NOMEM):
                    self._kick()
                    raise
                bad = True   # a shape the library refuses, no room for the staging: the host decodes this tile
            except Exception:
                self._kick()
                raise
            finally:   # the copy has run (or was never issued): the staging buffer goes back to the pool on every way out
                with self._cv:
                    self._pinned.append(arr.buf)
            if bad:  # a defective chunk: the host decodes the tile as it would have without the option, or raises as it would have
                self.fallbacks += 1
                try:
                    arr = self._decode(path)
                except Exception:
                    self._kick()
                    raise
            else:
                self.device_decodes += 1
                img = DeviceImage(dev, self._engine)
                self._current = (path, img)
                self._kick()
                return img
        t = arr if isinstance(arr, torch.Tensor) else torch.from_numpy(arr)
        dev = t.to(self._engine.device, non_blocking=True)
        buf = getattr(t, "_ze_pool_buffer", None)
        if buf is not None:  # the staging buffer goes back to the pool once the copy has run (checked at later calls)
            ev = torch.cuda.Event()
            ev.record(torch.cuda.current_stream(self._engine.device))
            self._in_copy.append((ev, buf))
        still = []
        for ev, b in self._in_copy:
            if ev.query():
                with self._cv:
                    self._pinned.append(b)
            else:
                still.append((ev, b))
        self._in_copy = still
        img = DeviceImage(dev, self._engine)
        self._current = (path, img)  # the previous tile's HBM is released with its last reference
        self._kick()
        return img
