"""Every driver form of qr.hip and every panel kernel of its units (qr_house.hip, qr_rowsplit.hip, qr_batched_panel.hip) through the device entry points (the batch reaches qr_choose as it is), against the
oracle on the same inputs. Every case asserts through qr_common.panel_plan(), the Python twin of the drivers, that it takes the path
it names (qr_common.CASES lists case -> kernels -> driver branch; test_qr_ref_host.py pins the twins on the CPU).

Inputs (qr_common.make_input): dense; graded (dense times 2^k_j, columns 2^+-100 apart inside every panel); and wherever a CholeskyQR2
panel runs (qrh_bc, qrb_panel) cond (a column delta away from another one in every panel, delta on either side of the fall-back
criterion), kahan and adv (U R0 with Kahan blocks / diag(1, delta, ..)(I - c strict_upper_ones) blocks on R0's diagonal: panels of
condition 1e3 ... 3e11 that pass the pivot test). One case per form also gets zero columns, a triangular input and a NaN.

Gates of every member with a reference (members 0, middle and last hold one matrix, the others a second one):
  shapes; R exactly upper triangular; guards either side of input and outputs intact, the input unchanged;
  colbe_gpu <= G colbe_oracle and orth_gpu <= G orth_oracle, colbe = max_j ||(Q R - A)[:, j]|| / ||a_j||, orth = max |Q^T Q - I| (and
  |Q Q^T - I| for a square Q), both sides by the same numpy code (torch fp64 on the device beyond 2000 rows);
  dense, graded: relerr <= 1e-12 of R and of the unique columns of Q against the oracle, and the sign conventions (M <= N or full:
  R_jj >= 0 for j < L - 1, det Q = +1 for square Q; tall: the leading minors of Q's top block are positive);
  graded: Q bit-identical to dense's, R bit-identical to dense's R times D;
  members 0, middle and last bit-identical; three calls in a row bit-identical (dense).

Measured on the MI355X (223 cases, 27 s in all; the slowest, the 8200-row global-memory panel, 2.2 s; all pass), GPU / oracle, worst
case of each family (colbe | orth), and by form look-ahead / batched / blocked / tall / TSQR for colbe:
  dense, graded    1.046 (bl_40) | 0.73     0.64 / 0.73 / 1.05 / 0.22 / 0.15     -> G = 4, the power of two at or above twice 1.046
  cond             0.65 | 0.73              0.64 / 0.65 / 0.59 / 0.15 / 0.10
  kahan            0.80 | 1.00              0.69 / 0.80 / 0.64 / 0.15 / 0.08
  adv              0.76 | 0.66              0.56 / 0.76 / 0.60 / 0.14 / 0.09
  panel entry point  0.48 | 1.00 (batched), 0.80 | 1.25 (row-split; the whole factor H: 0.92)
  relerr of Q and R against the oracle (dense, graded): at most 2.6e-14
(The inputs' seeds follow a case's position in qr_common.CASES: add new cases at the end, or measure again.)
Not reached by any case: more than 8 row workgroups per row-split panel (panels taller than 4080 rows in the tall form, where phase A
sums the partials beyond the eighth through qrh_sum_parts): the smallest such call, 4200 x 256 full, costs the oracle 7.7 s.
"""
import functools

import numpy as np
import pytest

import oracle
import qr_common as qc
from qr_common import CASES, EPS, SPECIAL_CASES

pytestmark = pytest.mark.gpu
G = 4.0              # see "Measured" above: the power of two at or above twice the worst dense / graded ratio (1.046)
BY_ID = {c["id"]: c for c in CASES}
BIG = 2000           # rows from which residual and orthogonality products are formed by torch on the device


def _mm(M):
    return qc.torch_matmul if M > BIG else np.matmul


def _oracle(a, full):
    with np.errstate(all="ignore"):
        return (oracle.qr_decomp_full if full else oracle.qr_decomp)(a)


@functools.lru_cache(maxsize=None)
def _input(cid, fam):
    a, other = qc.batch_input(BY_ID[cid], fam)
    a.setflags(write=False)
    return a, other


@functools.lru_cache(maxsize=None)
def _ref(cid, fam, member):
    """(colbe, orth, Q[:, :L], R) of the oracle on one member: one oracle factorisation per distinct input and module. graded: the
    oracle's factors of dense with R's columns scaled (bit for bit what the oracle returns: test_qr_ref_host.py), without a second run."""
    case = BY_ID[cid]
    a = _input(cid, fam)[0][member]
    M, N = a.shape
    L = min(M, N)
    if fam == "graded":
        q, r = _factors(cid, "dense", member)
        r = r * np.ldexp(1.0, qc.graded_exponents(N))
    else:
        q, r = _factors(cid, fam, member)
    sq = q.shape[-1] == M
    return qc.colbe(a, q, r, _mm(M)), qc.orth(q, both=sq, matmul=_mm(M)), q[:, :L].copy(), r[:L].copy()


@functools.lru_cache(maxsize=4)
def _factors(cid, fam, member):
    return _oracle(_input(cid, fam)[0][member], BY_ID[cid]["full"])


@functools.lru_cache(maxsize=2)
def _gpu(cid, fam):
    case = BY_ID[cid]
    return qc.call_qr(_input(cid, fam)[0], "full" if case["full"] else "decomp")


def _signs(a, q, r, full):
    M, N = a.shape
    L = min(M, N)
    d = np.diag(r)[:L]
    if M <= N or full:
        assert (d[:L - 1] >= 0).all()
        if q.shape[0] == q.shape[1] and M <= N:
            sign, _ = np.linalg.slogdet(q)
            assert sign == 1.0
    else:
        for k in range(1, min(N, 24) + 1):
            assert np.linalg.det(q[:k, :k]) > 0, k


def check_member(tag, cid, fam, member, q, r, unique=True):
    case = BY_ID[cid]
    a = _input(cid, fam)[0][member]
    M, N = a.shape
    L = min(M, N)
    cb_o, ob_o, q_o, r_o = _ref(cid, fam, member)
    assert qc.is_triu(r), tag
    cb = qc.colbe(a, q, r, _mm(M))
    ob = qc.orth(q, both=q.shape[-1] == M, matmul=_mm(M))
    print("%s member %d: colbe %.1f eps (oracle %.1f, ratio %.4f)  orth %.1f eps (oracle %.1f, ratio %.4f)"
          % (tag, member, cb / EPS, cb_o / EPS, cb / cb_o, ob / EPS, ob_o / EPS, ob / ob_o))
    assert cb <= G * cb_o and ob <= G * ob_o, (tag, member, cb / EPS, cb_o / EPS, ob / EPS, ob_o / EPS)
    if unique:
        eq, er = qc.relerr(q[:, :L], q_o), qc.relerr(r[:L], r_o[:L])
        print("%s member %d: relerr Q %.2e R %.2e" % (tag, member, eq, er))
        assert eq <= 1e-12 and er <= 1e-12, (tag, member, eq, er)
        _signs(a, q, r, case["full"])


def _bits(x, y):
    return x.shape == y.shape and np.array_equal(x.view(np.int64), y.view(np.int64))


PATH_PARAMS = [(c["id"], fam) for c in CASES for fam in qc.families_of(c, qc.panel_plan(c["batch"], c["M"], c["N"], c["full"]))]


@pytest.mark.parametrize("cid,fam", PATH_PARAMS, ids=["%s-%s" % p for p in PATH_PARAMS])
def test_path(cid, fam):
    case = BY_ID[cid]
    qc.check_plan(case)
    a, other = _input(cid, fam)
    b, M, N = a.shape
    L = min(M, N)
    q, r, intact = _gpu(cid, fam)
    qcols = M if case["full"] else L
    assert q.shape == (b, M, qcols) and r.shape == (b, qcols, N) and intact
    for member in [0] + ([other] if other is not None else []):
        check_member("%s-%s" % (cid, fam), cid, fam, member, q[member], r[member], unique=fam in ("dense", "graded"))
    for i in (b // 2, b - 1):                                                    # the same matrix anywhere in the batch
        assert _bits(q[i], q[0]) and _bits(r[i], r[0]), i
    if other is not None:
        for i in range(b):
            if i not in (0, b // 2, b - 1):
                assert _bits(q[i], q[other]) and _bits(r[i], r[other]), i
    if fam == "graded":                                                          # power-of-two column scaling commutes with every step
        qd, rd, _ = _gpu(cid, "dense")
        assert _bits(q, qd) and _bits(r, rd * np.ldexp(1.0, qc.graded_exponents(N)))
    if fam == "dense" and M <= 1100:                                             # stale tags in the exchange slots, workspace reuse
        for _ in range(2):
            q2, r2, ok = qc.call_qr(a, "full" if case["full"] else "decomp")
            assert ok and _bits(q2, q) and _bits(r2, r)


@pytest.mark.parametrize("cid", ["la_300x130", "la_257_qt", "b64_ragged", "bl_100", "tall_272"])
def test_inplace_form(cid):
    """dev.qr_decomp_inplace's entry point is the full form: the same R bit for bit, and Y <- Q^T Y"""
    case = BY_ID[cid]
    a, _ = _input(cid, "dense")
    b, M, N = a.shape
    assert qc.panel_plan(b, M, N, True)["form"] == case["expect"]["form"]
    y = qc.make_input("dense", 63000 + M, b * M, 3).reshape(b, M, 3)
    qf, rf, ok1 = qc.call_qr(a, "full")
    qty, r, ok2 = qc.call_qr(a, "inplace", y)
    assert ok1 and ok2 and _bits(r, rf)
    want = np.swapaxes(qf, -1, -2) @ y
    assert qc.relerr(qty, want) <= 1e-12


@pytest.mark.parametrize("cid", SPECIAL_CASES)
def test_triangular_input_is_returned_as_it_is(cid):
    case = BY_ID[cid]
    a, _ = qc.batch_input(case, "triu")
    b, M, N = a.shape
    q, r, intact = qc.call_qr(a, "full" if case["full"] else "decomp")
    qcols = q.shape[-1]
    assert intact
    for i in range(b):
        assert np.array_equal(q[i], np.eye(M)[:, :qcols]), i
        assert np.array_equal(r[i][:min(M, N)], a[i][:min(M, N)]) and not r[i][min(M, N):].any(), i


@pytest.mark.parametrize("cid", SPECIAL_CASES)
def test_zero_columns_do_not_disturb_their_neighbours(cid):
    case = BY_ID[cid]
    a, other = qc.batch_input(case, "zero")
    M, N = a.shape[-2:]
    q, r, intact = qc.call_qr(a, "full" if case["full"] else "decomp")
    assert intact
    zc = [c for c in (3, 21, N - 1) if c < N]
    for member in [0] + ([other] if other is not None else []):
        qo, ro = _oracle(a[member], case["full"])
        cb_o, ob_o = qc.colbe(a[member], qo, ro, _mm(M)), qc.orth(qo, both=qo.shape[-1] == M, matmul=_mm(M))
        cb, ob = qc.colbe(a[member], q[member], r[member], _mm(M)), qc.orth(q[member], both=q.shape[-1] == M, matmul=_mm(M))
        print("%s zero member %d: colbe %.1f / %.1f eps, orth %.1f / %.1f eps" % (cid, member, cb / EPS, cb_o / EPS, ob / EPS, ob_o / EPS))
        assert qc.is_triu(r[member]) and not r[member][:, zc].any()
        assert cb <= G * cb_o and ob <= G * ob_o, (cid, member, cb / EPS, cb_o / EPS, ob / EPS, ob_o / EPS)


@pytest.mark.parametrize("cid", SPECIAL_CASES + ("la_4x320_qt", "b_qrb41", "halves"))
def test_one_nan_stays_in_its_member(cid):
    case = BY_ID[cid]
    a = np.array(_input(cid, "dense")[0])
    b, M, N = a.shape
    kind = "full" if case["full"] else "decomp"
    q0, r0, _ = _gpu(cid, "dense")
    hit = 1 if b > 1 else 0
    a[hit, M // 2, min(5, N - 1)] = np.nan
    q, r, intact = qc.call_qr(a, kind)
    assert intact and np.isnan(r[hit]).any()
    for i in range(b):
        if i != hit:
            assert _bits(q[i], q0[i]) and _bits(r[i], r0[i]), i


# ------------------------------------------------------------------------------------------------------- the panel entry point
PANEL_KINDS = [("dense", 0), ("flagged", 0), ("kahan", 0), ("kahan", 1), ("kahan", 2), ("adv", 0), ("adv", 1), ("adv", 2), ("adv", 3)]
PANEL_SHAPES = [(1, 64), (1, 600), (1, 1100), (1, 2048), (8, 64), (8, 600), (8, 1100), (8, 2048),
                (9, 300), (9, 600), (9, 1100), (64, 200), (64, 400), (64, 900), (64, 1100)]


@functools.lru_cache(maxsize=None)
def _panel_ref(kind, which, M):
    a = qc.bare_panel(kind, 64000 + M, M, which)
    a.setflags(write=False)
    q, r = _oracle(a, False)
    oh = qc.orth(_oracle(a, True)[0], both=True) if M <= 1100 else None         # the oracle's full Q: what H is measured against
    return a, qc.colbe(a, q, r), qc.orth(q), oh


def _check_panel(tag, a, ref, r, v, t):
    """A = (I - V T V^T) [R; 0]: the first 16 columns Q16 = E - V (T V[:16]^T) of the orthogonal factor against the oracle's gates,
    and (up to 1100 rows) the orthogonality of the whole factor H against that of the oracle's full Q"""
    _, cb_o, ob_o, oh_o = ref
    M = a.shape[0]
    r = np.triu(r)
    q16 = np.eye(M)[:, :16] - v @ (t @ v[:16].T)
    cb, ob = qc.colbe(a, q16, r), qc.orth(q16)
    print("%s: colbe %.1f eps (oracle %.1f, ratio %.4f)  orth %.1f eps (oracle %.1f, ratio %.4f)"
          % (tag, cb / EPS, cb_o / EPS, cb / cb_o, ob / EPS, ob_o / EPS, ob / ob_o))
    assert cb <= G * cb_o and ob <= G * ob_o, (tag, cb / EPS, cb_o / EPS, ob / EPS, ob_o / EPS)
    if M <= 1100:
        h = np.eye(M) - v @ t @ v.T
        oh = np.abs(h.T @ h - np.eye(M)).max()
        print("%s: |H^T H - I| %.1f eps (oracle %.1f, ratio %.4f)" % (tag, oh / EPS, oh_o / EPS, oh / oh_o))
        assert oh <= G * oh_o, (tag, oh / EPS, oh_o / EPS)


@pytest.mark.parametrize("batch,M", PANEL_SHAPES, ids=["%dx%d" % s for s in PANEL_SHAPES])
def test_panel_entry_point(batch, M):
    """bare kahan and adv panels, a dense and a flagged member in every batch: both routes run in one launch; batches of 1 run every
    kind on its own. Members of one kind are bit-identical wherever they sit in the batch."""
    kernel, nwg = qc.panel_entry(batch, M)
    want = {(1, 64): ("qrh_bc<1>", 1), (1, 600): ("qrh_bc<2>", 2), (1, 1100): ("qrh_bc<4>", 3), (1, 2048): ("qrh_bc<4>", 5),
            (8, 64): ("qrh_bc<1>", 1), (8, 600): ("qrh_bc<2>", 2), (8, 1100): ("qrh_bc<4>", 3), (8, 2048): ("qrh_bc<4>", 5),
            (9, 300): ("qrb_panel<1,8>", 0), (9, 600): ("qrb_panel<2,8>", 0), (9, 1100): ("qrb_panel<4,8>", 0), (64, 200): ("qrb_panel<4,1>", 0),
            (64, 400): ("qrb_panel<4,2>", 0), (64, 900): ("qrb_panel<4,4>", 0), (64, 1100): ("qrb_panel<4,8>", 0)}
    assert (kernel, nwg) == want[(batch, M)]
    batches = [[k] for k in PANEL_KINDS] if batch == 1 else [[PANEL_KINDS[i % len(PANEL_KINDS)] for i in range(batch)]]
    for kinds in batches:
        a = np.stack([_panel_ref(k, w, M)[0] for k, w in kinds])
        r, v, t, intact = qc.call_panel(a)
        assert intact
        first = {}
        for i, (k, w) in enumerate(kinds):
            if (k, w) in first:
                j = first[(k, w)]
                assert _bits(r[i], r[j]) and _bits(v[i], v[j]) and _bits(t[i], t[j]), (i, j)
                continue
            first[(k, w)] = i
            _check_panel("panel %dx%d %s%d" % (batch, M, k, w), a[i], _panel_ref(k, w, M), r[i], v[i], t[i])
