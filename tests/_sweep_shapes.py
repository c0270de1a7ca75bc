"""The sweep shapes the library instantiates and the smallest problem that runs each of them (DESIGN.md "parity").

A sweep kernel exists once per pair (NV = 16-byte vectors per lane, LPC = lanes per row); the engine picks the pair from
the factor count and the dtype alone (policy.cpp choose_config).  This module holds, for tests/test_sweep_shapes_host.py
(which pins it against the library's own choose_config) and tests/test_sweep_shapes_gpu.py (which runs it):

  * SMALLEST_K: per plan and dtype, the smallest K of every pair -- the K with the most padding in the row's last vector;
  * the layouts a pair's kernels are reached through (workgroup size, balanced windows, half windows, entry format);
  * the smallest matrix on which a layout still has more than one block of major rows and more than one LDS window.

Never calls the device."""
import ctypes
import functools
import os
import re

import numpy as np

from conftest import ROOT, synthetic_counts

PLAN_CODE = {"auto": 0, "tile": 1, "gather": 2}
ITEMSIZE = {"float64": 8, "float32": 4}

TILE_PAIRS = ([(nv, 1) for nv in range(1, 8)] + [(nv, lpc) for lpc in (2, 4, 8) for nv in range(4, 8)] + [(4, 16)])
GATHER_PAIRS = ([(nv, 4) for nv in (1, 2, 3, 4, 5, 6, 7, 8, 10)] + [(nv, 8) for nv in (6, 7, 8, 10)]
                + [(nv, 16) for nv in (6, 7, 8)])
# float32 rows are half as long: 256 factors are 64 vectors, (8, 8); these gather pairs are instantiated and never chosen
GATHER_F32_UNREACHABLE = [(10, 8), (6, 16), (7, 16), (8, 16)]

# (plan, dtype) -> {(NV, LPC): smallest K}, in the order of the dispatch lists
SMALLEST_K = {
    ("tile", "float64"): dict(zip(TILE_PAIRS, [1, 3, 5, 7, 9, 11, 13, 15, 17, 21, 25, 29, 33, 41, 49, 57, 65, 81, 97, 113])),
    ("tile", "float32"): dict(zip(TILE_PAIRS, [1, 5, 9, 13, 17, 21, 25, 29, 33, 41, 49, 57, 65, 81, 97, 113, 129, 161, 193,
                                               225])),
    ("gather", "float64"): dict(zip(GATHER_PAIRS, [1, 9, 17, 25, 33, 41, 49, 57, 65, 81, 97, 113, 129, 161, 193, 225])),
    ("gather", "float32"): dict(zip([p for p in GATHER_PAIRS if p not in GATHER_F32_UNREACHABLE],
                                    [1, 17, 33, 49, 65, 81, 97, 113, 129, 161, 193, 225])),
}


def choose_config(dtype, K, plan):
    """The library's choose_config through schpf_debug_choose_config: {'tile', 'LPC', 'NV', 'KL', 'KP'}, or the
    library's message (a str) where it refuses."""
    from schpf_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int * 5)()
    code = _lib.F64 if np.dtype(dtype) == np.float64 else _lib.F32
    if lib.schpf_debug_choose_config(code, int(K), PLAN_CODE[plan], out):
        return lib.schpf_last_error().decode("utf-8", "replace")
    return dict(zip(("tile", "LPC", "NV", "KL", "KP"), [int(v) for v in out]))


def library_smallest_k(plan, dtype):
    """{(NV, LPC): smallest K in 1..256 for which the library picks the pair} under a forced plan, and the Ks it refuses."""
    first, refused = {}, []
    for K in range(1, 257):
        cfg = choose_config(dtype, K, plan)
        if isinstance(cfg, str):
            refused.append(K)
            continue
        assert cfg["tile"] == (plan == "tile")
        first.setdefault((cfg["NV"], cfg["LPC"]), K)
    return first, refused


def instantiated_pairs():
    """(tile pairs, gather pairs) as the dispatch macros of sweep_impl.h list them (the full build, not SCHPF_DEV_FAST)."""
    text = open(os.path.join(ROOT, "schpf_amd", "csrc", "sweep_impl.h")).read()
    full = text[text.index("#else", text.index("#ifdef SCHPF_DEV_FAST")):]
    full = full[:full.index("#endif")]
    tile_at, gather_at = full.index("#define SCHPF_DISPATCH_TILE("), full.index("#define SCHPF_DISPATCH(")
    assert tile_at < gather_at
    pairs = lambda s: [(int(a), int(b)) for a, b in re.findall(r"SCHPF_COMBO\((\d+), (\d+), CALLEXPR\)", s)]  # noqa: E731
    return pairs(full[tile_at:gather_at]), pairs(full[gather_at:])


# ---------------------------------------------------------------------------------------------------------- layouts
class Layout(object):
    """How a case reaches its kernels: the switches it sets and what plan_info() / upload_info() must then report."""

    def __init__(self, name, env, wpb, ring, packed):
        self.name, self.env, self.wpb, self.ring, self.packed = name, env, wpb, ring, packed
        self.lds_kib = 152 if wpb >= 12 else 64


def tile_layouts():
    out = []
    for name, env, wpb, ring, formats in (("t256", {"SCHPF_WPB": "4"}, 4, 1, (1, 0)),
                                          ("t1024", {"SCHPF_WPB": "16"}, 16, 1, (1, 0)),
                                          ("balanced", {"SCHPF_WPB": "16", "SCHPF_BALANCE": "1"}, 16, 1, (1, 0)),
                                          ("half", {"SCHPF_WPB": "16", "SCHPF_HALF": "2"}, 16, 2, (1,))):
        out += [Layout(name, env, wpb, ring, p) for p in formats]
    return out


def gather_layouts():
    # the gather plan has one entry format (32-bit index, float); "unpacked" is the same matrix as the tile cases'
    return [Layout("gather", {}, 0, 0, 1), Layout("gather", {}, 0, 0, 0)]


CLEARED = ("SCHPF_HALF", "SCHPF_BALANCE", "SCHPF_WPB", "SCHPF_LOSS_SIDE", "SCHPF_TASKS", "SCHPF_DUAL", "SCHPF_DEVICE_PLAN")
# layouts whose N is capped below a second window: pairs today's suite steps at many sizes (rows of 16 to 48 bytes)
SINGLE_WINDOW = {"t1024": [(1, 1), (2, 1), (3, 1)], "balanced": [(1, 1), (2, 1), (3, 1)], "half": [(1, 1)], "t256": [(1, 1)]}


class Case(object):
    def __init__(self, plan, dtype, pair, K, layout):
        self.plan, self.dtype, self.K, self.layout = plan, dtype, K, layout
        self.NV, self.LPC = pair
        self.N, self.G = matrix_shape(plan, pair, layout)
        self.id = "%s-%s-%dx%d-K%d-%s-%s" % (plan, "f64" if dtype == "float64" else "f32", self.NV, self.LPC, K,
                                             layout.name, "packed" if layout.packed else "unpacked")

    @property
    def win_rows(self):
        """rows of a whole LDS window (tile plan)"""
        return self.layout.lds_kib * 1024 // (self.NV * 16 * self.LPC)

    @property
    def several_windows(self):
        return (self.NV, self.LPC) not in SINGLE_WINDOW[self.layout.name]

    def matrix(self):
        return case_matrix(self.N, self.G, self.K, self.layout.packed)


def matrix_shape(plan, pair, layout):
    """The smallest (N, G) on which the shape has more than one block of major rows and more than one window in both
    orientations, N capped at 2600."""
    if plan == "gather":
        return 193, 217
    nv, lpc = pair
    block_rows = (64 // lpc) * layout.wpb
    win_rows = layout.lds_kib * 1024 // (nv * 16 * lpc)
    N = min(2600, max(block_rows, win_rows) + 41)
    return N, N + 24


@functools.lru_cache(maxsize=4)
def case_matrix(N, G, K, packed):
    X = synthetic_counts(N, G, min(0.12, 45000.0 / (N * G)), seed=K)
    if not packed:
        X.data[X.nnz // 2] = 70000       # one count beyond 16 bits: the 16-byte entry format
    for a in (X.data, X.row, X.col):
        a.setflags(write=False)
    return X


def cases(plan):
    """Every (dtype, pair, layout) of a plan at the pair's smallest K, layouts that share a matrix next to each other."""
    out = []
    for dtype in ("float64", "float32"):
        for pair, K in SMALLEST_K[(plan, dtype)].items():
            layouts = tile_layouts() if plan == "tile" else gather_layouts()
            for lay in sorted(layouts, key=lambda l: (l.wpb, -l.packed)):
                out.append(Case(plan, dtype, pair, K, lay))
    return out
