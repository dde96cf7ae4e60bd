"""The numpy / Python twin of rh_refit_component's definition (include/ransac_hip.h): cells by one binary64 subtraction,
division and floor, breadth-first search over a dict of cells, size in points, ties to the smallest point index.  Held to
hand-made cases written out here, to scipy.ndimage.label where scipy imports, and the ctypes bindings of the three new
entry points to the header's prototypes.  tests/test_component_gpu.py holds the device to this twin exactly."""
import ctypes as C
import itertools
import os
import re
from collections import deque

import numpy as np
import pytest

from ransac_jl_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFFS26 = [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]
OFFS6 = [d for d in OFFS26 if sum(abs(x) for x in d) == 1]


def ref_cells(xyz, idx, beta):
    """integer cells of the points idx (1-based) of xyz (n x 3 float64): floor((p - o) / beta), o their minimum"""
    p = np.asarray(xyz, dtype=np.float64)[np.asarray(idx, dtype=np.int64) - 1]
    o = p.min(axis=0)
    return np.floor((p - o) / np.float64(beta)).astype(np.int64)


def ref_labels(cells, conn26):
    """-> (label per point, number of components); labels number the components by their smallest point position"""
    assert cells.min() >= 0 and cells.max() < (1 << 20)
    key = (cells[:, 0] << 42) | (cells[:, 1] << 21) | cells[:, 2]      # one integer per cell: the unique pass is 1-D
    ukey, first, inv = np.unique(key, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    uniq = np.stack([ukey >> 42, (ukey >> 21) & 0x1FFFFF, ukey & 0x1FFFFF], axis=1)
    slot = {tuple(c): k for k, c in enumerate(uniq.tolist())}
    offs = OFFS26 if conn26 else OFFS6
    comp = np.full(len(uniq), -1, dtype=np.int64)
    ncomp = 0
    for k in np.argsort(first, kind="stable"):   # cells in the order their first point appears
        if comp[k] >= 0:
            continue
        comp[k] = ncomp
        todo = deque([uniq[k].tolist()])
        while todo:
            x, y, z = todo.popleft()
            for dx, dy, dz in offs:
                j = slot.get((x + dx, y + dy, z + dz))
                if j is not None and comp[j] < 0:
                    comp[j] = ncomp
                    todo.append([x + dx, y + dy, z + dz])
        ncomp += 1
    return comp[inv], ncomp


def ref_component(xyz, idx, beta, conn26):
    """-> (the points of idx, ascending 1-based, in the winning component; number of components)"""
    idx = np.asarray(idx, dtype=np.int64)
    assert np.all(np.diff(idx) > 0)
    if idx.size == 0:
        return idx.copy(), 0
    lab, ncomp = ref_labels(ref_cells(xyz, idx, beta), conn26)
    size = np.bincount(lab, minlength=ncomp)
    # labels are numbered by smallest point position: the first maximum is the tie-break of the definition
    return idx[lab == int(np.argmax(size))], ncomp


def _pts(*rows):
    return np.array(rows, dtype=np.float64)


def test_cells_by_the_formula():
    xyz = _pts([0.0, 0.0, 0.0], [0.25, 0.5, 0.75], [0.2, -0.25, 1.0], [-1.0, -0.25, 0.0])
    idx = np.arange(1, 5)
    # o = (-1, -0.25, 0); beta = 0.25: coordinates on cell faces belong to the upper cell
    assert ref_cells(xyz, idx, 0.25).tolist() == [[4, 1, 0], [5, 3, 3], [4, 0, 4], [0, 0, 0]]
    # a subset moves the origin
    assert ref_cells(xyz, [1, 2], 0.25).tolist() == [[0, 0, 0], [1, 2, 3]]
    # far from the origin: the same cells
    assert ref_cells(xyz + 1e6, idx, 0.25).tolist() == [[4, 1, 0], [5, 3, 3], [4, 0, 4], [0, 0, 0]]


def test_adjacency_corner_edge_face():
    a = [0.5, 0.5, 0.5]
    for b, joined26, joined6 in (([1.5, 1.5, 1.5], True, False), ([1.5, 1.5, 0.5], True, False), ([1.5, 0.5, 0.5], True, True),
                                 ([2.5, 0.5, 0.5], False, False)):
        xyz = _pts(a, b, b)          # two points in the second cell: it wins when the cells are apart
        for conn26, joined in ((True, joined26), (False, joined6)):
            got, n = ref_component(xyz, [1, 2, 3], 1.0, conn26)
            assert (got.tolist(), n) == (([1, 2, 3], 1) if joined else ([2, 3], 2))


def test_size_is_points_not_cells_and_ties_go_to_the_smallest_index():
    # 5 cells in a row with one point each, against one far cell with 6 points
    row = [[k + 0.5, 0.5, 0.5] for k in range(5)]
    far = [[20.5, 0.5, 0.5]] * 6
    got, n = ref_component(_pts(*(row + far)), np.arange(1, 12), 1.0, True)
    assert (got.tolist(), n) == ([6, 7, 8, 9, 10, 11], 2)
    # equal sizes: the component of point 1 wins although it sits at the larger coordinates
    xyz = _pts([9.5, 9.5, 9.5], [0.5, 0.5, 0.5], [0.5, 1.5, 0.5], [9.5, 8.5, 9.5])
    got, n = ref_component(xyz, [1, 2, 3, 4], 1.0, False)
    assert (got.tolist(), n) == ([1, 4], 2)
    # ... and among the listed points only: without point 1 the other component holds the smallest index
    xyz = _pts([9.5, 9.5, 9.5], [0.5, 0.5, 0.5], [0.5, 1.5, 0.5], [9.5, 8.5, 9.5], [9.5, 7.5, 9.5])
    got, n = ref_component(xyz, [2, 3, 4, 5], 1.0, False)
    assert (got.tolist(), n) == ([2, 3], 2)


def test_degenerate_sets():
    xyz = _pts([1.0, 2.0, 3.0], [1.0, 2.0, 3.0], [-4.0, 0.0, 0.0])
    assert ref_component(xyz, [], 0.5, True)[0].size == 0 and ref_component(xyz, [], 0.5, True)[1] == 0
    assert [x.tolist() if hasattr(x, "tolist") else x for x in ref_component(xyz, [3], 0.5, True)] == [[3], 1]
    assert [x.tolist() if hasattr(x, "tolist") else x for x in ref_component(xyz, [1, 2], 0.5, False)] == [[1, 2], 1]


def test_ring_and_negative_coordinates():
    # a ring of 8 cells around an empty centre: one component under either connectivity; the centre cell stays empty
    ring = [[x - 10.0, y - 10.0, -3.0] for x in range(3) for y in range(3) if (x, y) != (1, 1)]
    got, n = ref_component(_pts(*ring), np.arange(1, 9), 1.0, False)
    assert (got.tolist(), n) == (list(range(1, 9)), 1)
    # only the four corners: diagonal neighbours across the empty edge cells are two apart -- four components, the first wins
    corners = [[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.0, 2.0, 0.0], [2.0, 2.0, 0.0]]
    got, n = ref_component(_pts(*corners), [1, 2, 3, 4], 1.0, True)
    assert (got.tolist(), n) == ([1], 4)


@pytest.mark.parametrize("conn26", [True, False])
@pytest.mark.parametrize("seed", [0, 1])
def test_cell_labelling_against_scipy(conn26, seed):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(0, 20, size=(600, 3))     # 8000 cells, about 7 % occupied: many components under either connectivity
    idx = np.arange(1, 601)
    cells = ref_cells(xyz, idx, 1.0)
    lab, ncomp = ref_labels(cells, conn26)
    grid = np.zeros(cells.max(axis=0) + 1, dtype=bool)
    grid[tuple(cells.T)] = True
    structure = np.ones((3, 3, 3), dtype=bool) if conn26 else ndimage.generate_binary_structure(3, 1)
    slab, sn = ndimage.label(grid, structure=structure)
    assert sn == ncomp and ncomp > 3
    pairs = set(zip(lab.tolist(), slab[tuple(cells.T)].tolist()))
    assert len(pairs) == ncomp       # a bijection between the two labellings


_CTYPES = {"rh_cloud *": C.c_void_p, "const rh_cloud *": C.c_void_p, "const rh_shape *": C.POINTER(L.Shape),
           "const rh_params *": C.POINTER(L.Params), "double": C.c_double, "int32_t": C.c_int32, "int64_t": C.c_int64,
           "int64_t *": C.POINTER(C.c_int64), "int32_t *": C.POINTER(C.c_int32), "double *": C.POINTER(C.c_double)}


def test_bindings_match_the_header():
    hdr = open(os.path.join(ROOT, "include", "ransac_hip.h")).read()
    for name in ("rh_refit_component", "rh_cloud_set_component_filter", "rh_cloud_get_component_filter"):
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr)
        assert m, name
        args = []
        for a in m.group(1).split(","):
            t = re.sub(r"\s+", " ", re.sub(r"\w+$", "", a.strip())).strip()   # drop the parameter's name
            args.append(_CTYPES[t])
        res, got = L.SIGNATURES[name]
        assert res is C.c_int and got == args, name
    assert int(re.search(r"#define\s+RH_VERSION\s+(\d+)", hdr).group(1)) >= 111
