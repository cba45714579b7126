from emu_queries_ffi import load, radiance_samples  # noqa: F401  (the binding lives in emu_queries_ffi.py)
