"""ORACLE (test infrastructure only; never on the product path). ctypes wrapper around the exact sequential adjoint of
oracle/liboracle_seq.so (seq_adjoint.c): logpdf and its gradient with respect to the SHARED blocks of a Forward scalar-output
model, by reverse mode through the full recursion of seq_kalman.filter_ (time-varying covariance, no stationarity assumption).
Models use the dict convention of oracle/lgssm_ref.py (kind == 'scalar', ordering == 'F', every block shared: leading axis 1), d <= 64
(the kept steps take T (d^2 + d) long doubles: 0.8 GB at d = 9, T = 530 000; 0.1 GB at d = 63, T = 1500).
Returns the convention of temporalgps_jl_amd.lgssm.logpdf_adjoint: (lml, dict A (d,d), a (d,), Q (d,d), H (d,), h, R, x0m (d,),
x0P (d,d)); A, Q, x0P as [i][k]; the Q and x0P gradients symmetrised (pair them with symmetric tangents)."""
import ctypes

import numpy as np

from oracle import seq_kalman as sk

_i64 = ctypes.c_int64
_dp = ctypes.POINTER(ctypes.c_double)
_SIG_SET = False


def _lib():
    global _SIG_SET
    lib = sk.lib()
    if not _SIG_SET:
        lib.oracle_seq_adjoint.restype = ctypes.c_int
        lib.oracle_seq_adjoint.argtypes = [ctypes.c_int, _i64] + [_dp] * 9 + [ctypes.c_int] + [_dp] * 9
        lib.oracle_seq_adjoint_mant_dig.restype = ctypes.c_int
        lib.oracle_seq_adjoint_mant_dig.argtypes = []
        _SIG_SET = True
    return lib


def mant_dig():
    """mantissa bits of the arithmetic the reference build runs in (64 on x86-64)"""
    return int(_lib().oracle_seq_adjoint_mant_dig())


def logpdf_adjoint(model, y, use_double=False):
    assert model["kind"] == "scalar" and model["ordering"] == "F"
    d = len(model["x0m"])
    T = int(model["T"])
    for k in ("A", "a", "Q", "H"):
        assert np.asarray(model[k]).shape[0] == 1, f"{k}: the adjoint oracle takes shared blocks only"
    col = lambda M: np.ascontiguousarray(np.asarray(M, dtype=np.float64).T)       # row-major of M' == column-major of M
    A, Q, x0P = col(model["A"][0]), col(model["Q"][0]), col(model["x0P"])
    a, H = (np.ascontiguousarray(model[k][0], dtype=np.float64) for k in ("a", "H"))
    h, R = (np.ascontiguousarray(np.atleast_1d(model[k]), dtype=np.float64) for k in ("h", "R"))
    assert h.shape[0] == 1 and R.shape[0] == 1
    x0m = np.ascontiguousarray(model["x0m"], dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    assert y.shape == (T,)
    g = dict(A=np.zeros((d, d)), a=np.zeros(d), Q=np.zeros((d, d)), H=np.zeros(d), h=np.zeros(1), R=np.zeros(1), x0m=np.zeros(d), x0P=np.zeros((d, d)))
    lml = np.zeros(1)
    p = lambda arr: arr.ctypes.data_as(_dp)
    rc = _lib().oracle_seq_adjoint(d, _i64(T), p(A), p(a), p(Q), p(H), p(h), p(R), p(y), p(x0m), p(x0P), 1 if use_double else 0, p(lml),
                                   *[p(g[k]) for k in ("A", "a", "Q", "H", "h", "R", "x0m", "x0P")])
    assert rc == 0, rc
    for k in ("A", "Q", "x0P"):
        g[k] = g[k].T.copy()          # column-major blocks -> [i][k]
    g["h"], g["R"] = float(g["h"][0]), float(g["R"][0])
    return float(lml[0]), g
