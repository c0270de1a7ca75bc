"""The K -> sweep shape table of tests/_sweep_shapes.py against the library's own choose_config (through the host-only
hook schpf_debug_choose_config), and the matrices tests/test_sweep_shapes_gpu.py runs the shapes on.  No GPU."""
import ctypes

import numpy as np
import pytest

import _sweep_shapes as shapes


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("plan", ["tile", "gather"])
def test_smallest_k_of_every_pair_is_the_librarys(plan, dtype):
    first, refused = shapes.library_smallest_k(plan, dtype)
    assert first == shapes.SMALLEST_K[(plan, dtype)]
    assert list(first) == list(shapes.SMALLEST_K[(plan, dtype)])      # and found in the order of the dispatch list
    # rows beyond 1 KiB have no tile shape: a forced tile plan is refused from K = 129 in float64, never in float32
    assert refused == (list(range(129, 257)) if (plan, dtype) == ("tile", "float64") else [])


def test_pinned_smallest_k():
    """The table as numbers, so that a change of choose_config shows as a diff of this file too."""
    K = shapes.SMALLEST_K
    assert list(K[("tile", "float64")].values()) == [1, 3, 5, 7, 9, 11, 13, 15, 17, 21, 25, 29, 33, 41, 49, 57, 65, 81, 97, 113]
    assert list(K[("tile", "float32")].values()) == [1, 5, 9, 13, 17, 21, 25, 29, 33, 41, 49, 57, 65, 81, 97, 113, 129, 161,
                                                     193, 225]
    assert list(K[("gather", "float64")].values()) == [1, 9, 17, 25, 33, 41, 49, 57, 65, 81, 97, 113, 129, 161, 193, 225]
    assert list(K[("gather", "float32")].values()) == [1, 17, 33, 49, 65, 81, 97, 113, 129, 161, 193, 225]
    assert [lpc for (_, lpc), k in K[("gather", "float32")].items() if k >= 161] == [8, 8, 8]


def test_reached_pairs_are_the_instantiated_ones():
    tile, gather = shapes.instantiated_pairs()
    assert tile == shapes.TILE_PAIRS and gather == shapes.GATHER_PAIRS
    assert len(tile) == 20 and len(gather) == 16
    for dtype in ("float64", "float32"):
        assert list(shapes.library_smallest_k("tile", dtype)[0]) == tile
    assert list(shapes.library_smallest_k("gather", "float64")[0]) == gather
    # float32 rows of 256 factors are 64 vectors, (8, 8): four gather pairs are compiled and never chosen
    reached = list(shapes.library_smallest_k("gather", "float32")[0])
    assert [p for p in gather if p not in reached] == shapes.GATHER_F32_UNREACHABLE == [(10, 8), (6, 16), (7, 16), (8, 16)]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_the_library_picks_the_tile_plan_for_rows_up_to_1_kib(dtype):
    for K in range(1, 257):
        auto = shapes.choose_config(dtype, K, "auto")
        want = "tile" if K * shapes.ITEMSIZE[dtype] <= 1024 else "gather"
        assert auto == shapes.choose_config(dtype, K, want), K
        vec = 16 // shapes.ITEMSIZE[dtype]
        assert auto["KL"] == auto["NV"] * vec and auto["KP"] == auto["KL"] * auto["LPC"] and auto["KP"] >= K


def test_refusals_carry_the_librarys_message():
    assert "nfactors must be in [1, 256]" in shapes.choose_config("float64", 0, "auto")
    assert "nfactors must be in [1, 256]" in shapes.choose_config("float32", 257, "gather")
    assert "no instantiated sweep shape fits" in shapes.choose_config("float64", 129, "tile")
    from schpf_amd import _lib
    lib = _lib.load()
    assert lib.schpf_debug_choose_config(_lib.F64, 20, 0, None) != 0 and b"NULL" in lib.schpf_last_error()
    assert lib.schpf_debug_choose_config(7, 20, 0, (ctypes.c_int * 5)()) != 0
    assert lib.schpf_debug_choose_config(_lib.F64, 20, 3, (ctypes.c_int * 5)()) != 0


def test_case_list():
    tile, gather = shapes.cases("tile"), shapes.cases("gather")
    assert len(tile) == 40 * 7 and len(gather) == 28 * 2
    ids = [c.id for c in tile + gather]
    assert len(set(ids)) == len(ids)
    for c in tile:
        block_rows = (64 // c.LPC) * c.layout.wpb
        assert c.N == min(2600, max(block_rows, c.win_rows) + 41) and c.G == c.N + 24
        assert c.N > block_rows                                   # more than one block of major rows in both orientations
        assert c.several_windows == (c.N > (c.win_rows if c.layout.ring == 1 else c.win_rows // 2)), c.id
    assert min(c.N for c in tile) == 105 and max(c.N for c in tile) == 2600
    assert [c.id for c in tile if c.N == 105] == ["tile-f64-4x16-K113-t256-packed", "tile-f64-4x16-K113-t256-unpacked",
                                                  "tile-f32-4x16-K225-t256-packed", "tile-f32-4x16-K225-t256-unpacked"]
    assert sorted(set((c.NV, c.LPC, c.layout.name) for c in tile if not c.several_windows)) == sorted(
        [(1, 1, "t256"), (1, 1, "half")] + [(nv, 1, lay) for nv in (1, 2, 3) for lay in ("t1024", "balanced")])


def test_matrices_have_few_empty_rows_and_are_small():
    """Fewer than 5 % empty rows per axis (the cap of the per-row loss check), at most 55 000 stored entries, one count
    beyond 16 bits in the unpacked ones and none in the packed ones."""
    seen = set()
    for c in shapes.cases("tile") + shapes.cases("gather"):
        key = (c.N, c.G, c.K, c.layout.packed)
        if key in seen:
            continue
        seen.add(key)
        X = c.matrix()
        assert X.shape == (c.N, c.G) and 0 < X.nnz <= 55000
        assert (X.data > 65535).sum() == (0 if c.layout.packed else 1)
        for axis, idx, n in (("cell", X.row, c.N), ("gene", X.col, c.G)):
            empty = np.bincount(idx, minlength=n) == 0
            assert empty.mean() < 0.05, "%s: %d of %d rows by %s are empty" % (c.id, empty.sum(), n, axis)
        assert np.var(X.sum(1)) > 0 and np.var(X.sum(0)) > 0      # the empirical hyperparameters need a spread
