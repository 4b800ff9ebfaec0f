"""ctypes mirror of the host driver library (psmc_amd/host/libpsmc_host.so): the PSMC model -> HMM parameter map
(psmc_update_hmm, lh3/psmc core.c:61-133) for tools that need (a, e, a0) for a `PA` parameter vector -- bench.py's
parameter trajectory, scripts.  Plain host C, no GPU code."""
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
_dp = C.POINTER(C.c_double)


class _Pattern(C.Structure):
    _fields_ = [("n_states", C.c_int), ("n_free", C.c_int), ("group", C.POINTER(C.c_int))]


class _Model(C.Structure):  # psmc_model of psmc_amd/host/psmc_host.h, field for field
    _fields_ = [("pat", _Pattern), ("pattern_text", C.c_char_p), ("alpha", C.c_double), ("has_dt", C.c_int),
                ("fixed_t", C.POINTER(C.c_double)), ("n_params", C.c_int), ("params", C.POINTER(C.c_double)),
                ("t", C.POINTER(C.c_double)), ("sigma", C.POINTER(C.c_double)), ("post_sigma", C.POINTER(C.c_double)),
                ("C_pi", C.c_double), ("C_sigma", C.c_double),
                ("a", C.POINTER(C.c_double)), ("e", C.POINTER(C.c_double)), ("a0", C.POINTER(C.c_double)),
                ("lk", C.c_double), ("Q0", C.c_double), ("Q1", C.c_double), ("fast_mstep", C.c_int)]


def load():
    global _LIB
    if _LIB is None:
        p = os.path.join(_HERE, "host", "libpsmc_host.so")
        if not os.path.exists(p):
            raise RuntimeError("%s not built: run `make -C psmc_amd/host`" % p)
        lib = C.CDLL(p)
        lib.psmc_pattern_parse.argtypes = [C.c_char_p, C.POINTER(_Pattern)]
        lib.psmc_pattern_free.argtypes = [C.POINTER(_Pattern)]
        lib.psmc_model_new.restype = C.POINTER(_Model)
        lib.psmc_model_new.argtypes = [C.POINTER(_Pattern), C.c_char_p, C.c_double, C.c_int]
        lib.psmc_model_update.argtypes = [C.POINTER(_Model)]
        lib.psmc_model_free.argtypes = [C.POINTER(_Model)]
        lib.psmc_sample_host.argtypes = [C.c_int, _dp, _dp, _dp, C.POINTER(C.c_uint8), C.c_int32, C.c_uint64, C.c_uint64, C.c_int32,
                                         C.POINTER(C.c_int32)]
        _LIB = lib
    return _LIB


def sample_host(a, e, a0, seq, seed, stream_id, n_samp=1):
    """paths (n_samp, L) int32: psmc_sample_host, the plain C statement of the sampling definition of include/psmc_hip.h (forward
    filtering, backward sampling) for one segment; e is (2, n) or (3, n), rows hom, het."""
    lib = load()
    a = np.ascontiguousarray(a, dtype=np.float64)
    e = np.ascontiguousarray(np.asarray(e, dtype=np.float64)[:2])
    a0 = np.ascontiguousarray(a0, dtype=np.float64)
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    n = a0.shape[0]
    assert a.shape == (n, n) and e.shape == (2, n) and seq.ndim == 1 and len(seq) >= 1 and n_samp >= 1
    path = np.zeros((int(n_samp), len(seq)), dtype=np.int32)
    rc = lib.psmc_sample_host(n, a.ctypes.data_as(_dp), e.ctypes.data_as(_dp), a0.ctypes.data_as(_dp), seq.ctypes.data_as(C.POINTER(C.c_uint8)),
                              len(seq), int(seed) & (2 ** 64 - 1), int(stream_id) & (2 ** 64 - 1), int(n_samp), path.ctypes.data_as(C.POINTER(C.c_int32)))
    if rc:
        raise MemoryError("psmc_sample_host: %d" % rc)
    return path


def hmm_params(pattern, params, alpha=0.1):
    """(a (N,N), e (3,N), a0 (N,)) of the model with PA-line parameters [theta0, rho0, max_t, lambda_0 ..]."""
    lib = load()
    pat = _Pattern()
    if lib.psmc_pattern_parse(pattern.encode(), C.byref(pat)) != 0:
        raise ValueError("malformed pattern %r" % pattern)
    m = lib.psmc_model_new(C.byref(pat), pattern.encode(), alpha, 0)
    try:
        N, npar = pat.n_states, m.contents.n_params
        params = np.asarray(params, dtype=np.float64)
        if len(params) != npar:
            raise ValueError("pattern %s takes %d parameters, got %d" % (pattern, npar, len(params)))
        for i in range(npar):
            m.contents.params[i] = float(params[i])
        lib.psmc_model_update(m)
        a = np.ctypeslib.as_array(m.contents.a, shape=(N, N)).copy()
        e = np.ctypeslib.as_array(m.contents.e, shape=(3, N)).copy()
        a0 = np.ctypeslib.as_array(m.contents.a0, shape=(N,)).copy()
    finally:
        lib.psmc_model_free(m)
        lib.psmc_pattern_free(C.byref(pat))
    return a, e, a0
