"""Every function of the two headers that takes a `void *hip_stream` is a row of tests/test_gpu_stream_order.py's TABLE, and every row
names tests of that module: an entry point added later cannot go without a check on a stream of the caller's own."""
import os
import re

import test_gpu_stream_order as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = ("vecchio_amd.h", "vecchio_amd_debug.h")


def stream_taking_functions():
    found = set()
    for name in HEADERS:
        text = open(os.path.join(ROOT, "include", name)).read()
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)                       # comments speak of hip_stream too
        for m in re.finditer(r"\b(?:int|void|size_t)\s+(vk_\w+)\s*\(([^;{}]*?)\)\s*;", text, flags=re.S):
            if re.search(r"\bvoid\s*\*\s*hip_stream\b", m.group(2)):
                found.add(m.group(1))
    return found


def test_every_stream_taking_entry_point_is_a_row_of_the_table():
    declared = stream_taking_functions()
    assert len(declared) >= 13 and "vk_render_device" in declared and "vk_debug_trace_occluded_device" in declared, declared
    assert declared == set(T.TABLE), f"without a row: {sorted(declared - set(T.TABLE))}; rows of nothing: {sorted(set(T.TABLE) - declared)}"


def test_every_row_names_tests_that_exist_and_call_the_entry_point():
    source = open(T.__file__).read()
    wrappers = {"vk_debug_trace_occluded_device": "vk_debug_trace_occluded_device", "vk_temporal_accumulate_device": "accumulate_device",
                "vk_progress_step_device": "step_device", "vk_progress_stderr_device": "stderr_device"}
    for entry, tests in T.TABLE.items():
        assert tests, entry
        for t in tests:
            assert callable(getattr(T, t, None)) and t.startswith("test_"), (entry, t)
        call = wrappers.get(entry, entry[3:])                                    # (DeviceScene's wrapper carries the name without vk_)
        assert re.search(r"\b%s\(" % re.escape(call), source) or re.search(r"\b%s\(" % re.escape(entry), source), f"{entry} is never called"
