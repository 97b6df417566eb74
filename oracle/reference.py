"""ctypes binding of the compiled reference (TEST INFRASTRUCTURE ONLY): the reference's own src/kendallc.cpp built by
`make -C oracle ref` against oracle/rcpp_standin/Rcpp.h into oracle/_ref/.  Mirrors oracle/oracle.py.

Importable from tests/ and tests/golden/make_reference_golden.py and nowhere else; the product package never imports
it.  `available()` says whether the libraries exist or can be built (the reference's tree is present); nothing under
oracle/_ref/ is committed, so on a checkout without that tree and without a built oracle/_ref it is False.
"""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_REF = os.path.join(_HERE, "_ref")
_PATHS = {"plain": os.path.join(_REF, "libicikt_ref.so"), "wrapv": os.path.join(_REF, "libicikt_ref_wrapv.so")}
_SOURCES = ("ref_wrap.cpp", os.path.join("rcpp_standin", "Rcpp.h"), "Makefile")
REPORT_CAP = 4096

# label in the report the reference prints (output != "simple") -> the counts record's field name
REPORT_COUNTS = {"n_entry": "n", "missingness": "missing", "dis": "dis", "n_tie": "ntie", "x_tie": "xtie",
                 "y_tie": "ytie", "tot": "tot", "sum_obs": "sum_obs"}
# a word of each warning's text -> the reason code of include/icikt.h (reason 1, all missing, raises none)
_WARNING_REASON = (("single value", 2), ("unique", 3), ("Ties", 4))

_libs = {}


def reference_dir() -> str:
    return os.environ.get("ICIKT_REFERENCE_DIR", "/root/reference")


def _have_tree() -> bool:
    return os.path.exists(os.path.join(reference_dir(), "src", "kendallc.cpp"))


def _built() -> bool:
    return all(os.path.exists(p) for p in _PATHS.values())


def _stale() -> bool:
    newest = max(os.path.getmtime(os.path.join(_HERE, s)) for s in _SOURCES)
    return any(os.path.getmtime(p) < newest for p in _PATHS.values())


def available() -> bool:
    return _built() or _have_tree()


def build(force: bool = False) -> dict:
    if _have_tree() and (force or not _built() or _stale()):
        subprocess.run(["make", "-C", _HERE, "ref"] + (["-B"] if force else ["-s"]), check=True,
                       stdout=subprocess.DEVNULL)
    if not _built():
        raise RuntimeError("no compiled reference: neither oracle/_ref nor the reference's source tree "
                           f"({reference_dir()}) exists")
    return dict(_PATHS)


def lib(variant: str = "plain"):
    if variant not in _libs:
        L = ctypes.CDLL(build()[variant])
        dp = ctypes.POINTER(ctypes.c_double)
        ip = ctypes.POINTER(ctypes.c_int)
        L.ref_ici_kt.argtypes = [dp, dp, ctypes.c_long, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int,
                                 dp, ctypes.c_char_p, ctypes.c_long, ip]
        L.ref_ici_kt.restype = ctypes.c_int
        L.ref_last_warning.argtypes = [ctypes.c_char_p, ctypes.c_long]
        L.ref_last_warning.restype = None
        L.ref_count_rank_tie.argtypes = [dp, ctypes.c_long, dp]
        L.ref_count_rank_tie.restype = ctypes.c_int
        L.ref_kendall_discordant.argtypes = [ip, ip, ctypes.c_long]
        L.ref_kendall_discordant.restype = ctypes.c_int
        _libs[variant] = L
    return _libs[variant]


def _dp(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def parse_report(text: str) -> dict:
    """The report as {label: number}: `label: value` per line, the label cut at its first blank ("con_minus_dis
    (k_numerator)" -> "con_minus_dis"); integers stay ints, "%f" doubles become floats."""
    rep = {}
    for line in text.splitlines():
        key, sep, val = line.partition(":")
        if not sep:
            continue
        val = val.strip()
        try:
            rep[key.split(" ")[0].strip()] = int(val)
        except ValueError:
            rep[key.split(" ")[0].strip()] = float(val)
    return rep


def ici_kt(x, y, perspective="local", alternative="two.sided", continuity=False, want_report=True, variant="plain"):
    """The reference's ici_kt(): (out4, report dict -- empty when it returned before printing, number of warnings,
    reason code told from the warning's text: 0 none, 2 / 3 / 4, or 1 for all NA without a warning, the report's
    text as printed)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    if x.shape[0] != y.shape[0]:              # (the entry takes one length; the reference stops here as well)
        raise ValueError("'X' and 'Y' are not the same length!")
    out = np.full(4, -7.0)
    buf = ctypes.create_string_buffer(REPORT_CAP)
    n_warn = ctypes.c_int(0)
    L = lib(variant)
    rc = L.ref_ici_kt(_dp(x), _dp(y), x.shape[0], perspective.encode(), alternative.encode(), int(bool(continuity)),
                      int(bool(want_report)), _dp(out), buf, REPORT_CAP, ctypes.byref(n_warn))
    if rc:
        raise RuntimeError(buf.value.decode())
    report_text = buf.value.decode()
    reason = 0
    if n_warn.value:
        wbuf = ctypes.create_string_buffer(256)
        L.ref_last_warning(wbuf, 256)
        text = wbuf.value.decode()
        hits = [code for word, code in _WARNING_REASON if word in text]
        assert len(hits) == 1, text
        reason = hits[0]
    elif np.isnan(out).all():
        reason = 1
    return out, parse_report(report_text), n_warn.value, reason, report_text


def fill(x, y, perspective):
    """kendallc.cpp's treatment of the missing values, in numpy: "local" drops the rows missing in both, then each
    column's NaN become its minimum - 0.1.  Only the INPUT of ref_count_rank_tie is prepared here; the ranks and the
    sums are the reference's."""
    x = np.asarray(x, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    if perspective == "local":
        keep = ~(np.isnan(x) & np.isnan(y))
        x, y = x[keep], y[keep]
    x2 = np.where(np.isnan(x), x[~np.isnan(x)].min() - 0.1, x)
    y2 = np.where(np.isnan(y), y[~np.isnan(y)].min() - 0.1, y)
    return x2, y2


def count_rank_tie(col, variant="plain"):
    """(tie, t0, t1) of one filled column as ints, by the reference's sortedIndex / compare_self / cumsum /
    count_rank_tie."""
    col = np.ascontiguousarray(col, dtype=np.float64)
    assert not np.isnan(col).any()
    out = np.empty(3)
    rc = lib(variant).ref_count_rank_tie(_dp(col), col.shape[0], _dp(out))
    if rc:
        raise RuntimeError(f"ref_count_rank_tie failed rc={rc}")
    assert np.all(out == np.round(out))
    return tuple(int(v) for v in out)


def kendall_discordant(x4, y4, variant="plain"):
    x4 = np.ascontiguousarray(x4, dtype=np.int32)
    y4 = np.ascontiguousarray(y4, dtype=np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    return int(lib(variant).ref_kendall_discordant(x4.ctypes.data_as(ip), y4.ctypes.data_as(ip), x4.shape[0]))


def dense_ranks(x2, y2):
    """The (x4, y4) that ici_kt hands to kendall_discordant: rows in (x, y) order, dense ranks from 1."""
    order = np.lexsort((y2, x2))
    xs, ys = x2[order], y2[order]
    x4 = np.concatenate([[1], 1 + np.cumsum(xs[1:] != xs[:-1])]).astype(np.int32)
    y4 = (np.unique(ys, return_inverse=True)[1] + 1).astype(np.int32)
    return x4, y4


def counts(x, y, perspective="local", variant="plain", report=None):
    """The twelve count fields of oracle.COUNT_FIELDS from the reference: eight from its report, the six tie sums of
    the two columns from ref_count_rank_tie on the filled columns (xtie / ytie come both ways and must agree), `dis`
    once more from ref_kendall_discordant.  None when the reference returned before its report."""
    if report is None:
        report = ici_kt(x, y, perspective, variant=variant)[1]
    if not report:
        return None
    c = {field: report[label] for label, field in REPORT_COUNTS.items()}
    for k in ("ntie", "xtie", "ytie"):
        assert c[k] == int(c[k])
        c[k] = int(c[k])
    x2, y2 = fill(x, y, perspective)
    xt = count_rank_tie(x2, variant)
    yt = count_rank_tie(y2, variant)
    assert (xt[0], yt[0]) == (c["xtie"], c["ytie"]), (xt, yt, c)
    c.update(x0=xt[1], x1=xt[2], y0=yt[1], y1=yt[2])
    dis = kendall_discordant(*dense_ranks(x2, y2), variant=variant)
    assert dis == c["dis"], (dis, c["dis"])
    return c
