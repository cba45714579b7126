from emu_queries_ffi import load, trace_rays  # noqa: F401  (the binding lives in emu_queries_ffi.py)
