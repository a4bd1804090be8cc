"""CPU-side checks of the divide & conquer SVD: the host-computed level list that replaces the reference's recursion
(nd4hip_dbdsdc_levels, csrc/svd_dc.hip) against the recursion's own splits, and the argument errors of the Python hosts."""
import ctypes

import numpy as np
import pytest

import svd_dc_common as C
from nd4js_amd import _lib, la


def levels(n):
    lib = _lib.load()
    count = lib.nd4hip_dbdsdc_levels(n, None, 0)
    assert count > 0
    buf = (ctypes.c_int32 * (3 * count))()
    assert lib.nd4hip_dbdsdc_levels(n, buf, count) == count
    return [tuple(buf[3 * i:3 * i + 3]) for i in range(count)]


@pytest.mark.parametrize("n", range(2, 301))
def test_level_list_is_the_recursion(n):
    """same nodes as _svd_dc_bidiag visits (split at n >> 1, leaves of 2 and 3 columns); leaves are level 0; both children of a
    merge sit in an earlier level; the merges of a level are disjoint and differ in size by at most one"""
    got = levels(n)
    want = C.recursion_nodes(n)
    assert sorted((off, m) for _, off, m in got) == sorted((off, m) for off, m, _ in want)
    level_of = {(off, m): lv for lv, off, m in got}
    assert [lv for lv, _, _ in got] == sorted(lv for lv, _, _ in got)              # launch order = level order
    for off, m, leaf in want:
        if leaf:
            assert level_of[(off, m)] == 0
        else:
            n0 = m >> 1
            assert level_of[(off, m)] > max(level_of[(off, n0)], level_of[(off + n0, m - n0)])
    for lv in set(level_of.values()) - {0}:
        nodes = sorted((off, m) for l, off, m in got if l == lv)
        assert all(a[0] + a[1] <= b[0] for a, b in zip(nodes, nodes[1:]))
        sizes = [m for _, m in nodes]
        assert max(sizes) - min(sizes) <= 1
    assert max(level_of, key=lambda k: level_of[k]) == (0, n)                       # the root comes last


def test_level_list_arguments():
    lib = _lib.load()
    assert lib.nd4hip_dbdsdc_levels(1, None, 0) == -1
    assert b"nd4hip_dbdsdc_levels" in lib.nd4hip_last_error()
    buf = (ctypes.c_int32 * 3)()
    assert lib.nd4hip_dbdsdc_levels(9, buf, 1) == len(C.recursion_nodes(9))        # capacity limits what is written, not the count


def test_algo_argument_errors():
    from nd4js_amd import dev
    a = np.eye(4)
    for fn in (la.svd_decomp, dev.svd_decomp):
        for bad in ("qr", "DC", 1, ""):
            with pytest.raises(ValueError, match="algo must be None, 'jacobi' or 'dc'"):
                fn(a, algo=bad)
    assert la.svd_dc is la.svd_decomp and dev.svd_decomp.__defaults__ == (None, None)


def test_bidiag_svd_argument_errors():
    with pytest.raises(ValueError, match="len\\(d\\) - 1 or len\\(d\\)"):
        la.bidiag_svd(np.ones(4), np.ones(2))
    with pytest.raises(ValueError, match="len\\(d\\) - 1 or len\\(d\\)"):
        la.bidiag_svd(np.ones(4), np.ones(5))
    with pytest.raises(ValueError, match="same leading dimensions"):
        la.bidiag_svd(np.ones((2, 4)), np.ones((3, 4)))
    with pytest.raises(TypeError):
        la.bidiag_svd(np.ones(4, dtype=np.float32), np.ones(3))
