"""uvx_llm_ws_bytes is pinned: over Llama, Qwen3-style, Gemma and Gemma-3 configurations, with and without llm_wt_stream, both dtypes, with and
without the backward's buffers, at (B, T) = (1, 1), (3, 80) and (8, 320), it returns exactly what tests/golden/llm_ws_bytes.json recorded
(tests/golden/make_golden.py llm_ws_bytes_cases; tiny widths and the Llama-3-8B shape).  The sizes are host arithmetic: no GPU."""
import ctypes
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def _grid():
    # the generator's own grid, read from its source without running the module (its imports need the reference tree)
    src = open(os.path.join(HERE, "golden", "make_golden.py")).read()
    start, end = src.index("LLM_WS_SHAPES = {"), src.index("def llm_ws_bytes_cases")
    ns = {}
    exec(compile(src[start:end], "make_golden.py", "exec"), ns)
    return list(ns["llm_ws_bytes_grid"]())


def test_llm_workspace_sizes_are_pinned():
    from ultravox_amd import _lib
    lib = _lib.lib()
    want = json.load(open(os.path.join(HERE, "golden", "llm_ws_bytes.json")))
    grid = _grid()
    assert len(grid) == len(want) == 4 * 2 * 2 * 2 * 3 + 2 * 2 * 2 * 3 and {k for k, *_ in grid} == set(want)
    got = {key: int(lib.uvx_llm_ws_bytes(ctypes.byref(_lib.Config(**fields)), B, T, save)) for key, fields, B, T, save in grid}
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, wrong
    assert all(v > 256 for v in want.values())
