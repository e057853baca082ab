"""Near-duplicate images: which FILES hold the same picture -- a re-save at another size, a JPEG of a PNG, a second download?

Beyond the reference, which has no such step.  Two device stages (include/hip_tagsearch.h states the definitions):

  image_hashes      a 128-bit gradient hash of the model-input tensor uint8 [n,S,S,3] (hipts_image_hash_u8, csrc/imghash.hip): Pillow's
                    grey, cell means of an 8 x 9 and a 9 x 8 grid compared exactly in integers; word 0 holds the horizontal
                    comparisons, word 1 the vertical ones.
  ImageHashIndex    paths + hashes; `neighbors` is the relation  popcount(h_i ^ h_j) <= max_distance  over all pairs as CSR lists
                    (hipts_radius_create_hamming, csrc/radius.hip), `groups` its connected components (hipts_radius_dbscan with
                    min_samples = 2).

Everything is integer arithmetic: the results are exact and the same bytes run to run.
"""
import ctypes
from typing import List, Sequence, Tuple

import numpy as np

from . import _lib

CHUNK = 256                  # images per hipts_image_hash_u8 call: 154 MB of uint8 at 448
MIN_SIZE, MAX_SIZE = 9, 1024


def image_hashes(images, device: int = 0) -> np.ndarray:
    """uint64 [n, 2] hashes of uint8 [n,S,S,3] images: a numpy array, or a torch tensor (host or device memory) the way the decode pool
    hands it over.  Any n (n = 0 gives an empty array); the library is called for CHUNK images at a time."""
    is_np = isinstance(images, np.ndarray)
    if not is_np and not hasattr(images, "data_ptr"):
        images = np.asarray(images)
        is_np = True
    shape = tuple(images.shape)
    if len(shape) != 4 or shape[1] != shape[2] or shape[3] != 3:
        raise ValueError("images must be uint8 [n,S,S,3], got shape %r" % (shape,))
    if is_np:
        if images.dtype != np.uint8:
            raise ValueError("images must be uint8, got %s" % images.dtype)
    elif "uint8" not in str(images.dtype):
        raise ValueError("images must be uint8, got %s" % images.dtype)
    n = shape[0]
    out = np.empty((n, 2), dtype=np.uint64)
    if n == 0:
        return out
    space = _lib.HOST if is_np else _lib.memspace_of(images)
    if space == _lib.DEVICE and images.device.index != device:
        raise ValueError("the images live on device %d, not on device %d" % (images.device.index, device))
    stream = _lib.current_stream_ptr()
    for s in range(0, n, CHUNK):
        part = images[s:s + CHUNK]
        part = np.ascontiguousarray(part) if is_np else part.contiguous()
        # host output: the call has synchronised when it returns, `part` may go
        _lib.call("hipts_image_hash_u8", _lib.ptr(part), space, int(part.shape[0]), int(shape[1]), _lib.ptr(out[s:s + CHUNK]), _lib.HOST,
                  int(device), stream)
    return out


def set_bits(hashes: np.ndarray) -> np.ndarray:
    """int64 [n]: how many of a hash's 128 bits are set.  A flat picture (an all-white page) has none."""
    h = np.ascontiguousarray(hashes, dtype=np.uint64).reshape(-1, 2)
    return np.unpackbits(h.view(np.uint8).reshape(len(h), 16), axis=1).sum(axis=1).astype(np.int64)


class ImageHashIndex:
    """Paths and their hashes, row aligned.  save / load: `prefix.npy` (uint64 [n, 2]) and `prefix.csv` (one path per line)."""

    def __init__(self, device: int = 0):
        self.device = device
        self.paths: List[str] = []
        self.hashes = np.empty((0, 2), dtype=np.uint64)

    def __len__(self) -> int:
        return len(self.paths)

    def add(self, paths: Sequence[str], hashes) -> None:
        hashes = np.ascontiguousarray(hashes, dtype=np.uint64).reshape(-1, 2)
        paths = list(paths)
        if len(paths) != len(hashes):
            raise ValueError("%d paths but %d hashes" % (len(paths), len(hashes)))
        self.paths.extend(paths)
        self.hashes = np.concatenate([self.hashes, hashes])

    def save(self, prefix: str) -> None:
        np.save(prefix + ".npy", self.hashes)
        with open(prefix + ".csv", "w", encoding="utf-8") as f:
            f.write("".join(p + "\n" for p in self.paths))

    @classmethod
    def load(cls, prefix: str, device: int = 0) -> "ImageHashIndex":
        index = cls(device)
        hashes = np.load(prefix + ".npy")
        with open(prefix + ".csv", encoding="utf-8") as f:
            paths = [line.rstrip("\n") for line in f]
        if hashes.dtype != np.uint64 or hashes.ndim != 2 or hashes.shape[1] != 2:
            raise ValueError("%s.npy must be uint64 [n, 2], got %s %r" % (prefix, hashes.dtype, hashes.shape))
        index.add(paths, hashes)
        return index

    def _relation(self, hashes: np.ndarray, max_distance: int, max_pairs: int):
        h = ctypes.c_void_p()
        hashes = np.ascontiguousarray(hashes, dtype=np.uint64)
        _lib.call("hipts_radius_create_hamming", _lib.ptr(hashes), _lib.HOST, ctypes.c_int64(len(hashes)), int(max_distance),
                  ctypes.c_int64(int(max_pairs)), int(self.device), _lib.current_stream_ptr(), ctypes.byref(h))
        return h

    def neighbors(self, max_distance: int = 10, max_pairs: int = 0) -> Tuple[np.ndarray, np.ndarray]:
        """(ptr int64 [n + 1], ids int32 [pairs]): ids[ptr[i]:ptr[i + 1]] are, ascending, the rows j whose hash differs from row i's
        in at most max_distance of the 128 bits -- the raw relation over ALL rows, row i itself among them.  max_pairs: the call
        refuses (HipTagSearchError naming the count) when more pairs than this are in the relation; 0 = what fits in half of the free
        device memory.  An empty index is refused."""
        h = self._relation(self.hashes, max_distance, max_pairs)
        try:
            rows, pairs = ctypes.c_int64(), ctypes.c_int64()
            _lib.call("hipts_radius_info", h, ctypes.byref(rows), ctypes.byref(pairs))
            ptr = np.empty(rows.value + 1, dtype=np.int64)
            ids = np.empty(pairs.value, dtype=np.int32)
            _lib.call("hipts_radius_read", h, _lib.ptr(ptr), _lib.ptr(ids))
        finally:
            _lib.call("hipts_radius_destroy", h)
        return ptr, ids

    def groups(self, max_distance: int = 10, min_set_bits: int = 8, max_pairs: int = 0) -> np.ndarray:
        """labels int32 [n]: the connected components of the rows that have at least one other neighbour, numbered from 0 by their
        smallest row; every row without a neighbour gets -1.  Rows whose hash has fewer than min_set_bits set bits -- flat pictures,
        which would all pair with each other -- are left out before the device call and get -1 too (min_set_bits = 0: none is)."""
        n = len(self.paths)
        labels = np.full(n, -1, dtype=np.int32)
        keep = np.flatnonzero(set_bits(self.hashes) >= int(min_set_bits))
        if len(keep) == 0:
            return labels
        h = self._relation(self.hashes[keep], max_distance, max_pairs)
        try:
            sub = np.empty(len(keep), dtype=np.int32)
            clusters, sweeps = ctypes.c_int64(), ctypes.c_int32()
            _lib.call("hipts_radius_dbscan", h, 2, _lib.ptr(sub), ctypes.byref(clusters), ctypes.byref(sweeps))
        finally:
            _lib.call("hipts_radius_destroy", h)
        # `keep` ascends: the smallest kept row of a component is also its smallest row, so the numbering carries over as it is
        labels[keep] = sub
        return labels
