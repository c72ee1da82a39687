"""Posterior quantiles on the CPU: the host driver of the radix selection (glabcmcmc_amd.diagnostics.select) fed by the NumPy
restatement of glabc_key_counts (tests/quantile_ref.py) against numpy.sort and numpy.quantile, the restatement's histogram
against numpy.histogram, every ValueError of the new functions, and the refusals of glabc_key_counts / glabc_histogram as
csrc/glabc_check.h answers them under g++.

Comparisons of order statistics and counts are exact: equal integers, and equal float32 values with NaN matching NaN.
"""
import numpy as np
import pytest

import diag_ref as R
import quantile_ref as Q
from glabcmcmc_amd import diagnostics as D
from test_arg_checks import check_table

OK, NULL, DIM, ARG = 0, -1, -2, -4


def same_values(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def ref_counter(hist, calls=None):
    def count_fn(level, prefixes):
        if calls is not None:
            calls.append((level, None if prefixes is None else np.array(prefixes)))
        return Q.key_counts(hist, level, prefixes)
    return count_fn


def ranks_of(n):
    return [0, 1, n // 4, n // 2, n - 2, n - 1]


def nine_ranks(n):
    return sorted({(i * (n - 1)) // 8 for i in range(9)})


def inputs():
    special = Q.special_values()
    return [("diag_history", R.diag_history(97, 3, 321)), ("special", np.ascontiguousarray(special.reshape(-1, 1, 1))),
            ("special tiled", Q.special_history(33, 2, 65))]


def sorted_columns(hist):
    return np.stack([np.sort(hist[:, j].reshape(-1)) for j in range(hist.shape[1])], axis=1)          # [N][d]


# ---------------------------------------------------------------------------------- the key
def test_key_orders_as_sort_and_unkey_inverts():
    v = Q.special_values()
    k = Q.keys(v)
    assert k[0] == k[1] == 0x80000000                                   # -0 and +0 are one value
    assert (k[np.isnan(v)] == 0xFFFFFFFF).all()
    order = np.argsort(k, kind="stable")
    assert same_values(v[order], np.sort(v))
    back = Q.unkey(k)
    assert same_values(back, v) and not np.signbit(back[1])            # -0 comes back as +0.0
    assert same_values(D.unkey(k), back)
    x = R.diag_history(97, 3, 321).reshape(-1)
    assert (np.diff(Q.keys(np.sort(x)).astype(np.int64)) >= 0).all() and same_values(Q.unkey(Q.keys(x)), x)


# ---------------------------------------------------------------------------------- the driver against sort
@pytest.mark.parametrize("name, hist", inputs(), ids=[n for n, _ in inputs()])
def test_select_equals_sort(name, hist):
    s = sorted_columns(hist)
    n = s.shape[0]
    assert len(nine_ranks(n)) == 9
    for ranks in (ranks_of(n), nine_ranks(n), [n // 2], [n - 1, 0, 0]):
        calls = []
        got = D.select(ref_counter(hist, calls), ranks=ranks)
        assert got.dtype == np.float32 and got.shape == (len(ranks), hist.shape[1])
        assert same_values(got, s[ranks]), (name, ranks)
        assert [c[0] for c in calls] == [0, 1, 2]                       # one call per level
        for level, table in calls[1:]:
            for row in table:                                           # deduplicated, distinct, unused slots behind
                used = row[row != Q.UNUSED]
                assert len(set(used.tolist())) == len(used) and (used >> Q.LEVELS[level][0] == 0).all()
    # nine distinct ranks of well-spread data walk more than 8 prefixes: the split over launches is the counter's business
    calls = []
    D.select(ref_counter(R.diag_history(97, 3, 321), calls), ranks=nine_ranks(97 * 321))
    assert calls[2][1].shape[1] == 9


def test_level0_digit_count_of_the_inputs():
    """what the contention discussion of DESIGN.md 4.5 quotes: diag_history hits 115 level-0 digits, a constant one"""
    c = Q.key_counts(R.diag_history(97, 3, 321), 0)
    assert int((c.sum(axis=(0, 1)) > 0).sum()) == 115
    assert int((Q.key_counts(np.full((5, 1, 7), 2.5, np.float32), 0) > 0).sum()) == 1


def test_shards_add_up():
    hist = R.diag_history(97, 3, 321)
    a, b = hist[:, :, :130], hist[:, :, 130:]

    def both(level, prefixes):
        return Q.key_counts(a, level, prefixes) + Q.key_counts(b, level, prefixes)
    n = 97 * 321
    ranks = ranks_of(n) + nine_ranks(n)
    assert same_values(D.select(both, ranks=ranks), D.select(ref_counter(hist), ranks=ranks))
    assert same_values(D.select(both, ranks=ranks), sorted_columns(hist)[ranks])
    q = (0.025, 0.5, 0.975)
    assert same_values(D.select(both, q=q), D.select(ref_counter(hist), q=q))


# ---------------------------------------------------------------------------------- quantiles
QS = (0.0, 0.025, 0.1, 0.25, 1.0 / 3.0, 0.5, 0.75, 0.975, 0.999, 1.0)


def test_quantile_matches_the_formula_and_numpy():
    """Exactly the restatement's formula; within 4 ulps of max(|x_lo|, |x_hi|) of numpy.quantile on the float64 values (NumPy's
    lerp rounds one product and one sum, possibly from the other end: 2 ulps is the bound, 4 leaves a factor of two)"""
    hist = R.diag_history(97, 3, 321)
    got = D.select(ref_counter(hist), q=QS)
    assert got.dtype == np.float64 and got.shape == (len(QS), 3)
    assert np.array_equal(got, Q.quantile(hist, QS))
    s = sorted_columns(hist).astype(np.float64)
    n = s.shape[0]
    for i, q in enumerate(QS):
        lo = int(np.floor(q * (n - 1)))
        hi = min(lo + 1, n - 1)
        bound = 4 * np.spacing(np.maximum(np.abs(s[lo]), np.abs(s[hi])))
        err = np.abs(got[i] - np.quantile(s, q, axis=0))
        print("q = %.4f: largest |select - numpy.quantile| / bound = %.3g" % (q, (err / bound).max()))
        assert (err <= bound).all(), (q, err, bound)
    assert np.array_equal(D.select(ref_counter(hist), q=0.5), got[5:6])           # a scalar q is one row


def test_quantile_of_data_with_a_nan_is_nan():
    hist = np.array(R.diag_history(33, 2, 65))
    hist[7, 1, 3] = np.nan
    got = D.select(ref_counter(hist), q=(0.0, 0.5, 1.0))
    assert np.isnan(got[:, 1]).all() and np.array_equal(got[:, 0], Q.quantile(hist, (0.0, 0.5, 1.0))[:, 0])
    assert same_values(got, Q.quantile(hist, (0.0, 0.5, 1.0)))
    with np.errstate(invalid="ignore"):
        assert np.isnan(np.quantile(hist[:, 1].astype(np.float64), 0.5))


# ---------------------------------------------------------------------------------- the restatement's histogram against NumPy
@pytest.mark.parametrize("lo, hi", [(0, 16), (-7, 9), (3, 4), (-64, 64)])
def test_restatement_histogram_matches_numpy(lo, hi):
    """integers in float32, integer lo / hi, bins = hi - lo: the bin arithmetic is exact, so the counts must be NumPy's"""
    rng = np.random.default_rng([lo + 100, hi + 100])
    x = rng.integers(lo - 3, hi + 4, (40, 2, 23)).astype(np.float32)
    x[0, 0, :5] = hi                                                   # x == hi lands in the last bin
    x[1, 1, :5] = lo
    bins = hi - lo
    got = Q.histogram(x, bins, [lo, lo], [hi, hi])
    for j in range(2):
        v = x[:, j].reshape(-1)
        want, _ = np.histogram(v, bins=bins, range=(lo, hi))
        assert np.array_equal(got[j, :bins], want.astype(np.uint64))
        assert got[j, bins] == (v < lo).sum() and got[j, bins + 1] == (v > hi).sum() and got[j, bins + 2] == 0
        assert got[j].sum() == v.size
    assert got[0, bins - 1] >= 5
    x[2, 0, 0] = np.nan
    assert Q.histogram(x, bins, [lo, lo], [hi, hi])[0, bins + 2] == 1


# ---------------------------------------------------------------------------------- argument errors, no GPU needed
def test_argument_errors_come_before_any_device(monkeypatch):
    from glabcmcmc_amd import engine

    def no_device(*a, **k):
        raise AssertionError("an argument error must be raised before the device is asked for")
    monkeypatch.setattr(engine, "require_device", no_device)
    ok = np.zeros((10, 3, 2), np.float32)                                             # N = 30
    for q in (-0.1, 1.5, np.nan, (0.5, 2.0), [[0.5]]):
        with pytest.raises(ValueError):
            D.quantile(ok, q)
        with pytest.raises(ValueError):
            D.select(ref_counter(ok.transpose(0, 2, 1)), q=q)
    for ranks in (-1, 30, (0, 31), 2.5, [[1]]):
        with pytest.raises(ValueError):
            D.order_statistics(ok, ranks)
    for ranks in (-1, 30, 2.5):                                                       # 30: known once the level-0 counts are in
        with pytest.raises(ValueError):
            D.select(ref_counter(ok.transpose(0, 2, 1)), ranks=ranks)
    with pytest.raises(ValueError):
        D.select(ref_counter(ok))
    with pytest.raises(ValueError):
        D.select(ref_counter(ok), ranks=[0], q=[0.5])
    for prob in (0.0, 1.0, -0.5, 1.5, np.nan):
        with pytest.raises(ValueError):
            D.interval(ok, prob)
    for bins in (0, -1, 4097, 2.5, True):
        with pytest.raises(ValueError):
            D.histogram(ok, bins)
    for rng in ((1.0, 1.0), (2.0, 1.0), (0.0, np.inf), (np.nan, 1.0), (0.0, 1.0, 2.0), 3.0, np.zeros((3, 2)), "ab"):
        with pytest.raises(ValueError):
            D.histogram(ok, 8, rng)
    for level, prefixes in ((3, None), (-1, None), (0.5, None), (0, [[1, 2]] * 2), (1, None), (1, [[1]]), (1, [[1], [1 << 11]]),
                            (2, [[1 << 22], [0]]), (1, [[5, 5], [1, 2]]), (1, [[0.5], [1.0]]), (1, [[-1], [1]])):
        with pytest.raises(ValueError):
            D.key_counts(ok, level, prefixes)
    for call in (lambda h: D.quantile(h, 0.5), lambda h: D.order_statistics(h, 0), D.interval, D.histogram, lambda h: D.key_counts(h, 0)):
        for bad in (np.zeros(5, np.float32), np.zeros((5, 2, 2, 2), np.float32), np.zeros((10, 3, 9), np.float32)):
            with pytest.raises(ValueError):
                call(bad)
    with pytest.raises(ValueError):
        D.quantile(ok, 0.5, layout="columns")


def test_no_cpu_fallback():
    """Without a GPU the new functions raise; they never compute on the host"""
    import torch
    if not torch.cuda.is_available():
        ok = np.zeros((10, 3, 2), np.float32)
        for call in (lambda: D.quantile(ok, 0.5), lambda: D.order_statistics(ok, 0), lambda: D.interval(ok), lambda: D.histogram(ok),
                     lambda: D.histogram(ok, 8, (0.0, 1.0)), lambda: D.key_counts(ok, 0)):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                call()


def test_entry_points_are_bound():
    from glabcmcmc_amd import _capi
    assert "glabc_key_counts" in _capi.ENTRY_POINTS and "glabc_histogram" in _capi.ENTRY_POINTS
    assert _capi.VERSION == 301
    assert D.KEY_LEVELS == Q.LEVELS and D.MAX_PREFIXES == 8 and D.MAX_BINS == 4096 and D.UNUSED_PREFIX == Q.UNUSED


# ---------------------------------------------------------------------------------- the refusals (csrc/glabc_check.h)
PRELUDE_TABLES = ("static const uint32_t P1[24] = {5, 6, 7, 8, 9, 10, 11, 12, 1, 2, 3, 4, 5, 6, 7, 8, 0, 2047, 3, 4, 5, 6, 7, 8}; "
                  "static const uint32_t DUP[6] = {1, 2, 3, 4, 5, 3}; static const uint32_t DUP_LATER[6] = {1, 2, 3, 7, 5, 7}; static const uint32_t DUP_UNUSED[6] = {1, 0xFFFFFFFFu, 0xFFFFFFFFu, 4, 5, 6}; "
                  "static const uint32_t WIDE1[3] = {1, 2, 2048}; static const uint32_t WIDE2[3] = {1, 1u << 22, 3}; "
                  "static const uint32_t TOP2[3] = {(1u << 22) - 1, 0, 0xFFFFFFFFu}; static uint64_t CNT[4]; "
                  "static const double LO[3] = {-1.0, 0.0, 5.0}, HI[3] = {1.0, 1e-300, 6.0}; "
                  "static const double BAD_EQ[3] = {-1.0, 1e-300, 5.0}, BAD_NAN[3] = {-1.0, NAN, 5.0}, BAD_INF[3] = {-1.0, 0.0, -INFINITY}, "
                  "HI_INF[3] = {1.0, INFINITY, 6.0}, BAD_REV[3] = {2.0, 0.0, 5.0}; ")


def test_check_key_counts(tmp_path_factory):
    call = "check_key_counts(%s, %s, %s, %s, %s, %s, %s, %s, %s)"
    base = dict(h="b.f", rows="97", d="3", n="65", stride="65", level="1", np="1", p="P1", c="CNT")

    def row(want, **kw):
        a = dict(base, **kw)
        return (PRELUDE_TABLES, call % (a["h"], a["rows"], a["d"], a["n"], a["stride"], a["level"], a["np"], a["p"], a["c"]), want)
    check_table(tmp_path_factory, "key_counts", [
        row(OK), row(OK, np="8"), row(OK, level="2", np="8"), row(OK, level="0"), row(OK, level="0", p="WIDE2"),          # ignored at level 0
        row(OK, rows="1"), row(OK, stride="82"), row(OK, n="0", stride="0"), row(OK, d="1"), row(OK, d="8", p="b.u", np="1", level="0"),
        row(OK, d="1", np="6", p="DUP_UNUSED"),                          # unused slots may repeat
        row(OK, d="1", np="3", level="2", p="TOP2"), row(OK, d="1", np="3", level="2", p="WIDE1"),
        row(NULL, h="nullptr"), row(NULL, p="nullptr"), row(NULL, c="nullptr"), row(NULL, p="nullptr", level="0"),
        row(NULL, h="nullptr", d="0"), row(NULL, c="nullptr", level="7"),          # a null pointer is reported first
        row(DIM, d="0"), row(DIM, d="9"), row(DIM, d="-1"), row(DIM, d="9", rows="0"), row(DIM, d="0", level="3"),          # then the dimension
        row(ARG, rows="0"), row(ARG, rows="-5"), row(ARG, n="-1"), row(ARG, stride="64"),
        row(ARG, level="-1"), row(ARG, level="3"),
        row(ARG, np="0"), row(ARG, np="9"), row(ARG, np="-1"), row(ARG, level="0", np="2"), row(ARG, level="0", np="0"),
        row(ARG, d="1", np="3", p="WIDE1"), row(ARG, d="1", np="3", level="2", p="WIDE2"), row(ARG, d="1", np="3", level="1", p="TOP2"),
        row(ARG, d="1", np="6", p="DUP"), row(ARG, d="2", np="3", p="DUP_LATER"), row(OK, d="2", np="3", p="DUP"), row(OK, d="3", np="2", p="DUP"),          # equal within one coordinate only
    ])


def test_check_histogram(tmp_path_factory):
    call = "check_histogram(%s, %s, %s, %s, %s, %s, %s, %s, %s)"
    base = dict(h="b.f", rows="97", d="3", n="65", stride="65", bins="64", lo="LO", hi="HI", c="CNT")

    def row(want, **kw):
        a = dict(base, **kw)
        return (PRELUDE_TABLES, call % (a["h"], a["rows"], a["d"], a["n"], a["stride"], a["bins"], a["lo"], a["hi"], a["c"]), want)
    check_table(tmp_path_factory, "histogram", [
        row(OK), row(OK, bins="1"), row(OK, bins="4096"), row(OK, rows="1"), row(OK, stride="82"), row(OK, n="0", stride="0"), row(OK, d="1"),
        row(OK, d="2", lo="BAD_INF"),                                    # the third coordinate is not looked at
        row(NULL, h="nullptr"), row(NULL, lo="nullptr"), row(NULL, hi="nullptr"), row(NULL, c="nullptr"),
        row(NULL, h="nullptr", d="0"), row(NULL, c="nullptr", bins="0"),          # a null pointer is reported first
        row(DIM, d="0"), row(DIM, d="9"), row(DIM, d="-1"), row(DIM, d="9", rows="0"), row(DIM, d="0", bins="0"),          # then the dimension
        row(ARG, rows="0"), row(ARG, rows="-5"), row(ARG, n="-1"), row(ARG, stride="64"),
        row(ARG, bins="0"), row(ARG, bins="-1"), row(ARG, bins="4097"),
        row(ARG, lo="BAD_EQ"), row(ARG, lo="BAD_NAN"), row(ARG, hi="BAD_NAN"), row(ARG, lo="BAD_INF"), row(ARG, hi="HI_INF"),
        row(ARG, lo="BAD_REV"), row(ARG, lo="HI", hi="LO"),
    ])


# ---------------------------------------------------------------------------------- the committed resource report
def test_resource_report_shows_no_private_segment():
    """profiles/quant_kernel_resources.txt: every instantiation of count_kernel without a private segment or a spilled register,
    at eight wavefronts per SIMD, so that the workgroups of eight wavefronts a CU's LDS holds are resident together"""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "profiles", "quant_kernel_resources.txt")).read()
    kernels = re.split(r"^Function Name: ", text, flags=re.M)[1:]
    assert len(kernels) >= 3 and all("count_kernel" in k for k in kernels)
    assert any("KeySlots" in k for k in kernels) and any("HistSlots" in k for k in kernels)
    for k in kernels:
        field = lambda name: int(re.search(r"%s: (\d+)" % re.escape(name), k).group(1))          # noqa: E731
        assert field("ScratchSize [bytes/lane]") == 0 and field("VGPRs Spill") == 0 and field("SGPRs Spill") == 0
        assert field("VGPRs") + field("AGPRs") <= 64 and field("Occupancy [waves/SIMD]") >= 8
