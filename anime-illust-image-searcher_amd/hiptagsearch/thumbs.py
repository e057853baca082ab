"""Thumbnails and contact sheets: the project writes pictures, not only text.

Beyond the reference, which answers a query by opening every full-size original per page view (webui.py display_images).  The JPEG
encode is the hybrid decode's mirror image (include/hip_tagsearch.h states the definitions):

  jpeg_encode       uint8 [n,H,W,3] RGB -> the files PIL.Image.save(..., "JPEG", quality=Q) writes, byte for byte.  Colour conversion,
                    chroma downsampling, forward DCT and quantisation on the device (hipts_jpeg_encode_batch_u8, csrc/jpegenc.hip) into
                    coefficient slots; one copy to pinned host memory; Huffman coding in plain C on a few host threads
                    (hipts_jpeg_entropy_encode of libhipts_jpeg_host.so, called through ctypes: the interpreter lock is released).
  ThumbnailWriter   a thumbnail cache of the collection, made from the model-input tensor uint8 [n,S,S,3] -- the padded white square the
                    tagger sees and find_duplicates.py hashes, so every input mode gives the same bytes for the same picture.  A thumbnail
                    is Image.fromarray(x).resize((size, size), Image.BICUBIC) saved at `quality`; files go to
                    out_dir/<first two hex digits>/<sha1 of the utf-8 path>.jpg, and out_dir/thumbnails.csv lists `path,relative
                    thumbnail path`, appended in order and flushed per batch.
  contact_sheet     one JPEG that shows what a query found: existing thumbnails, decoded by the hybrid decoder, row-major on a white
                    canvas in device memory, encoded once.

Everything is integer arithmetic: the same bytes run to run.
"""
import concurrent.futures
import ctypes
import hashlib
import os
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib

MAX_THREADS = 16
CSV_NAME = "thumbnails.csv"
_HEADER_BYTES = 1024                     # csrc/jpeg_slot.h
_FILE_HEAD_BYTES = 640                   # markers and tables in front of the entropy-coded data (623) and EOI, rounded up
_host = None


def _host_lib():
    global _host
    if _host is None:
        from . import pipeline
        _host = pipeline.load_jpeg_host_lib()
    return _host


def _threads(threads: int) -> int:
    return max(1, min(int(threads), MAX_THREADS))


def _as_device_images(images, device: int):
    """uint8 [n,H,W,3] (numpy array, or torch tensor in host or device memory) -> contiguous torch tensor on `device`"""
    import torch
    if isinstance(images, np.ndarray) or not hasattr(images, "data_ptr"):
        images = np.ascontiguousarray(images)
        if images.dtype != np.uint8:
            raise ValueError("images must be uint8, got %s" % images.dtype)
        images = torch.from_numpy(images)
    if images.dtype != torch.uint8:
        raise ValueError("images must be uint8, got %s" % images.dtype)
    if images.dim() != 4 or images.shape[3] != 3:
        raise ValueError("images must be uint8 [n,H,W,3], got shape %r" % (tuple(images.shape),))
    if images.is_cuda and images.device.index != device:
        raise ValueError("the images live on device %d, not on device %d" % (images.device.index, device))
    return images.to("cuda:%d" % device).contiguous()


def slot_total_bytes(height: int, width: int) -> int:
    """bytes of the 4:2:0 slot the encoder writes: the header and six blocks per 16 x 16 MCU"""
    return _HEADER_BYTES + ((width + 15) // 16) * ((height + 15) // 16) * 6 * 128


class _Launched:
    """a batch on its way: the slots in pinned host memory once `event` has passed"""

    def __init__(self, slots, event, n: int, total: int):
        self.slots, self.event, self.n, self.total = slots, event, n, total


def _launch(images, quality: int, device: int, pinned=None, dev_slots=None) -> _Launched:
    """device encode of a device tensor uint8 [n,H,W,3] on the current stream + the copy of the slots to pinned host memory; nothing waits.
    pinned / dev_slots: buffers to reuse (at least as large as needed)."""
    import torch
    n, h, w = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
    lib = _lib.load()
    stride = int(lib.hipts_jpeg_slot_bytes(w, h))
    total = slot_total_bytes(h, w)
    with torch.cuda.device(device):
        if dev_slots is None or dev_slots.numel() < n * stride:
            dev_slots = torch.empty(n * stride, dtype=torch.uint8, device="cuda:%d" % device)
        if pinned is None or pinned.numel() < n * total:
            pinned = torch.empty(n * total, dtype=torch.uint8).pin_memory()
        _lib.call("hipts_jpeg_encode_batch_u8", _lib.ptr(images), _lib.DEVICE, n, h, w, int(quality), _lib.ptr(dev_slots), _lib.DEVICE,
                  ctypes.c_int64(stride), int(device), _lib.current_stream_ptr())
        host = pinned[:n * total].view(n, total)
        host.copy_(dev_slots[:n * stride].view(n, stride)[:, :total], non_blocking=True)     # the one copy: the used part of every slot
        event = torch.cuda.Event()
        event.record(torch.cuda.current_stream(device))
    out = _Launched(host, event, n, total)
    out.buffers = (pinned, dev_slots)
    return out


def _code_one(slot_address: int, total: int) -> bytes:
    """hipts_jpeg_entropy_encode of one slot.  The first try offers as many bytes as the slot has (files are a fraction of that); a file that
    does not fit gets the worst case: 27 bits per coefficient, every byte stuffed."""
    lib = _host_lib()
    nb = ctypes.c_int64(0)
    for capacity in (total, _FILE_HEAD_BYTES + (total - _HEADER_BYTES) // 128 * 64 * 7):
        out = np.empty(capacity, dtype=np.uint8)
        status = lib.hipts_jpeg_entropy_encode(ctypes.c_void_p(slot_address), ctypes.c_int64(total), out.ctypes.data_as(ctypes.c_void_p),
                                               ctypes.c_int64(capacity), ctypes.byref(nb))
        if status == 0:
            return out[:nb.value].tobytes()
        if status != 2:
            break
    raise RuntimeError("hipts_jpeg_entropy_encode: status %d" % status)


def _code(launched: _Launched, executor) -> List[bytes]:
    launched.event.synchronize()
    base = launched.slots.data_ptr()
    return list(executor.map(lambda i: _code_one(base + i * launched.total, launched.total), range(launched.n)))


def jpeg_encode(images, quality: int = 85, device: int = 0, threads: int = 8) -> List[bytes]:
    """The files PIL.Image.fromarray(images[i]).save(..., "JPEG", quality=quality) writes, for uint8 [n,H,W,3] RGB images (numpy, or torch in
    host or device memory) of 16 .. 8192 pixels either way."""
    images = _as_device_images(images, device)
    if images.shape[0] == 0:
        return []
    launched = _launch(images, quality, device)
    with concurrent.futures.ThreadPoolExecutor(max_workers=_threads(threads)) as ex:
        return _code(launched, ex)


def thumbnail_relpath(path: str) -> str:
    """<first two hex digits>/<sha1 of the utf-8 path>.jpg"""
    h = hashlib.sha1(path.encode("utf-8")).hexdigest()
    return "%s/%s.jpg" % (h[:2], h)


def read_index(out_dir: str) -> Dict[str, str]:
    """thumbnails.csv of a ThumbnailWriter: path -> thumbnail file (the last line of a path counts)"""
    index = {}
    with open(os.path.join(out_dir, CSV_NAME), "r", encoding="utf-8") as f:
        for line in f:
            line = line.rstrip("\n")
            if "," in line:
                path, rel = line.rsplit(",", 1)
                index[path] = os.path.join(out_dir, rel)
    return index


class ThumbnailWriter:
    """add(paths, images_u8) per batch of model-input images; close() when done (or use it as a context manager).

    add() only launches: resize (hipts_resize_batch_u8: Pillow's bicubic, skipped when size == S), encode and the copy to pinned memory go
    on the current stream, and the batch is handed to a thread that waits for the copy, runs the host coder on `threads` threads, writes
    the files and appends the csv lines, in order.  While it does, the caller launches the next batch; two batches can be on their way."""

    def __init__(self, out_dir: str, size: int = 256, quality: int = 85, device: int = 0, threads: int = 8):
        if size % 16 != 0 or not 64 <= size <= 512:
            raise ValueError("size must be a multiple of 16 in 64..512, got %r" % (size,))
        if not 1 <= quality <= 100:
            raise ValueError("quality must be in 1..100, got %r" % (quality,))
        self.out_dir, self.size, self.quality, self.device = out_dir, int(size), int(quality), int(device)
        os.makedirs(out_dir, exist_ok=True)
        self._csv = open(os.path.join(out_dir, CSV_NAME), "a", encoding="utf-8")
        self._coders = concurrent.futures.ThreadPoolExecutor(max_workers=_threads(threads))
        self._writer = concurrent.futures.ThreadPoolExecutor(max_workers=1)      # one: files and csv lines keep the order of add()
        self._buffers = [(None, None), (None, None)]
        self._pending = [None, None]
        self._step = 0
        self._dirs = set()
        self.count = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _finish(self, paths: List[str], launched: _Launched, keep) -> None:
        files = _code(launched, self._coders)
        lines = []
        for path, data in zip(paths, files):
            rel = thumbnail_relpath(path)
            sub = rel[:2]
            if sub not in self._dirs:
                os.makedirs(os.path.join(self.out_dir, sub), exist_ok=True)
                self._dirs.add(sub)
            with open(os.path.join(self.out_dir, rel), "wb") as f:
                f.write(data)
            lines.append("%s,%s\n" % (path, rel))
        self._csv.write("".join(lines))
        self._csv.flush()
        del keep            # the device tensors the launches read

    def add(self, paths: Sequence[str], images_u8) -> None:
        import torch
        paths = list(paths)
        images = _as_device_images(images_u8, self.device)
        if images.shape[1] != images.shape[2]:
            raise ValueError("model-input images are square, got shape %r" % (tuple(images.shape),))
        if len(paths) != images.shape[0]:
            raise ValueError("%d paths but %d images" % (len(paths), images.shape[0]))
        if not paths:
            return
        slot = self._step & 1
        if self._pending[slot] is not None:
            self._pending[slot].result()           # the batch that used these buffers two add()s ago
        n, S = int(images.shape[0]), int(images.shape[1])
        thumbs = images
        with torch.cuda.device(self.device):
            if S != self.size:
                thumbs = torch.empty((n, self.size, self.size, 3), dtype=torch.uint8, device=images.device)
                hw = np.full((n, 2), S, dtype=np.int32)
                _lib.call("hipts_resize_batch_u8", _lib.ptr(images), _lib.DEVICE, ctypes.c_int64(S * S * 3), _lib.ptr(hw), n, 0, _lib.ptr(thumbs),
                          self.size, 3, self.device, _lib.current_stream_ptr())
            pinned, dev_slots = self._buffers[slot]
            launched = _launch(thumbs, self.quality, self.device, pinned, dev_slots)
        self._buffers[slot] = launched.buffers
        self._pending[slot] = self._writer.submit(self._finish, paths, launched, (images, thumbs))
        self._step += 1
        self.count += n

    def close(self) -> None:
        """waits for the batches on their way; raises what one of them raised"""
        try:
            for k in (self._step & 1, (self._step + 1) & 1):          # older first
                if self._pending[k] is not None:
                    self._pending[k].result()
                    self._pending[k] = None
        finally:
            self._writer.shutdown(wait=True)
            self._coders.shutdown(wait=True)
            if not self._csv.closed:
                self._csv.close()


def _decode_thumbnail(path: Optional[str], size: int, device: int, out) -> bool:
    """a thumbnail file -> `out` (device uint8 [size,size,3]) through the hybrid decoder; False: missing, not decodable, or another size"""
    if not path:
        return False
    try:
        with open(path, "rb") as f:
            data = f.read()
    except OSError:
        return False
    lib = _host_lib()
    nbytes = int(lib.hipts_jpeg_slot_bytes(size, size))
    slot = np.empty(nbytes, dtype=np.uint8)
    arr = np.frombuffer(data, dtype=np.uint8)
    if len(arr) < 4 or lib.hipts_jpeg_entropy_decode(arr.ctypes.data_as(ctypes.c_void_p), ctypes.c_int64(len(arr)), slot.ctypes.data_as(ctypes.c_void_p),
                                                     ctypes.c_int64(nbytes)) != 0:
        return False                   # (a larger picture does not fit the slot: status 2)
    width, height = (int(v) for v in slot[8:16].view(np.int32))
    if width != size or height != size:
        return False
    try:
        _lib.call("hipts_jpeg_decode_rgb", _lib.ptr(slot), ctypes.c_int64(nbytes), _lib.ptr(out), _lib.DEVICE, ctypes.c_int64(size * size * 3),
                  int(device), _lib.current_stream_ptr())
    except _lib.HipTagSearchError as e:
        if e.status != -1:             # an argument the library refuses is this file's trouble; anything else is not
            raise
        return False
    return True


def contact_sheet(thumb_paths: Sequence[Optional[str]], columns: int = 8, size: int = 256, quality: int = 85, device: int = 0,
                  threads: int = 8) -> bytes:
    """One JPEG of the thumbnails `thumb_paths` (files of a ThumbnailWriter of this `size`), row-major, `columns` per row, on white: what
    Image.new("RGB", (columns * size, rows * size), "white") with Image.open(thumb) pasted per cell gives when saved at `quality`.  A path
    that is None, missing or not decodable leaves its cell white."""
    import torch
    if columns < 1:
        raise ValueError("columns must be at least 1, got %r" % (columns,))
    thumb_paths = list(thumb_paths)
    rows = max(1, (len(thumb_paths) + columns - 1) // columns)
    with torch.cuda.device(device):
        canvas = torch.full((rows * size, columns * size, 3), 255, dtype=torch.uint8, device="cuda:%d" % device)
        cell = torch.empty((size, size, 3), dtype=torch.uint8, device="cuda:%d" % device)
        for i, path in enumerate(thumb_paths):
            if _decode_thumbnail(path, size, device, cell):
                r, c = divmod(i, columns)
                canvas[r * size:(r + 1) * size, c * size:(c + 1) * size] = cell
        return jpeg_encode(canvas[None], quality, device, threads)[0]
