"""ctypes binding of libmreserve_ingest.so (include/mreserve_ingest.h).  As with _lib there is NO fallback: if the library is
missing or a call fails, this raises."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'libmreserve_ingest.so')

i64, i32, f32, vp = C.c_int64, C.c_int32, C.c_float, C.c_void_p
DT_S16, DT_F32 = 0, 1

# name -> (restype, argtypes); every symbol declared in include/mreserve_ingest.h
PROTOTYPES = {
    'mri_version': (i32, []),
    'mri_last_error': (C.c_char_p, []),
    'mri_resample_len': (i64, [i64, i64, i64]),
    'mri_resample_mono': (i32, [vp, i32, i64, i64, i64, i64, vp, i64, i64, i64, vp, vp, vp]),
    'mri_content_bounds': (i32, [vp, i64, i64, i64, i32, vp, vp]),
}

_lib = None


class MreserveIngestError(RuntimeError):
    pass


def load():
    """Load the library (once).  Raises if it has not been built: run `python -m merlot_reserve_amd.build`."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MreserveIngestError(f'{LIB_PATH} not found: the HIP extension is not built '
                                  f'(python -m merlot_reserve_amd.build). There is no CPU fallback.')
    import torch  # noqa: F401      (its HIP runtime must be in the process first, as for _lib)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)       # AttributeError if a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().mri_last_error()
        raise MreserveIngestError(f'{what} failed ({rc}): {msg.decode() if msg else ""}')
