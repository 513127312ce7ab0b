"""A compact fixture format for many small arrays (tests/golden/ref_*.npz, written by oracle/gen_golden_ref.py).

Values that a test compares within a tolerance are stored as they are, concatenated into one float64 and one float32
array.  Values that a test requires to be exactly equal (initial parameters, confusion matrices, labels) are stored as
a digest of their shape and values (``digest``): equal digests mean equal arrays, so no copy is needed.  Lists of names
are stored as lists.  The index, in the order the entries were added, is one JSON string.
"""
from __future__ import annotations

import hashlib
import json
from collections import OrderedDict

import numpy as np


def digest(a) -> str:
    """sha256 of an array's shape and values.  Values are compared as float64 with -0.0 taken as 0.0, so two arrays
    with equal finite values (np.array_equal / torch.equal) have the same digest whatever their storage type."""
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    v = np.ascontiguousarray(a.astype(np.float64) + 0.0)
    return hashlib.sha256(repr(tuple(a.shape)).encode() + v.tobytes()).hexdigest()


def save(path: str, values: dict, exact: dict, lists: dict, meta: dict) -> None:
    """values: name -> float64 / float32 array (kept); exact: name -> array (digest only); lists: name -> list."""
    index = {"arrays": OrderedDict(), "digests": OrderedDict(), "lists": lists, "meta": meta}
    parts = {"f64": [], "f32": []}
    size = {"f64": 0, "f32": 0}
    for name, a in values.items():
        a = np.asarray(a)
        kind = "f64" if a.dtype == np.float64 else "f32"
        if a.dtype not in (np.float64, np.float32):
            raise TypeError(f"{name}: {a.dtype} (values are float64 or float32)")
        index["arrays"][name] = [kind, size[kind], list(a.shape)]
        parts[kind].append(a.reshape(-1))
        size[kind] += a.size
    for name, a in exact.items():
        index["digests"][name] = digest(a)
    np.savez_compressed(path, f64=np.concatenate(parts["f64"] or [np.zeros(0)]).astype(np.float64),
                        f32=np.concatenate(parts["f32"] or [np.zeros(0, np.float32)]).astype(np.float32),
                        index=np.array(json.dumps(index)))


class Packed:
    def __init__(self, path: str):
        with np.load(path) as z:
            self._buf = {"f64": z["f64"], "f32": z["f32"]}
            self._index = json.loads(str(z["index"]))

    @property
    def meta(self) -> dict:
        return self._index["meta"]

    def __getitem__(self, name: str) -> np.ndarray:
        kind, off, shape = self._index["arrays"][name]
        n = int(np.prod(shape)) if shape else 1
        return self._buf[kind][off: off + n].reshape(shape)

    def under(self, prefix: str) -> "OrderedDict[str, np.ndarray]":
        """The stored arrays named ``prefix/<rest>``, as {rest: array}, in the order they were written."""
        p = prefix + "/"
        return OrderedDict((k[len(p):], self[k]) for k in self._index["arrays"] if k.startswith(p))

    def digests_under(self, prefix: str) -> "OrderedDict[str, str]":
        p = prefix + "/"
        return OrderedDict((k[len(p):], d) for k, d in self._index["digests"].items() if k.startswith(p))

    def matches(self, name: str, a) -> bool:
        """``a`` equals the array recorded (as a digest) under ``name``."""
        return digest(a) == self._index["digests"][name]

    def list(self, name: str) -> list:
        return self._index["lists"][name]
