from emu_queries_ffi import irradiance_samples, load  # noqa: F401  (the binding lives in emu_queries_ffi.py)
