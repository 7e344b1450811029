"""Coverage guard for the f32 parity-mode kernel tests (no GPU needed): every compute entry point of include/uvx.h that takes
a dtype - an `int32_t dtype` argument, or a config struct that carries one - must be called in f32 by
tests/test_f32_kernels_gpu.py, unless it is a whole-model entry point listed below.  A dtype-taking kernel added later
without an f32 test fails here."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Whole-model entry points: their f32 paths (and the kernels reached only through them - LoRA, decode attention, KV-cache
# append, wav2vec2) are covered end to end against the f32 CPU oracle by test_f32_parity_gpu.py, test_c2_full_depth_gpu.py,
# test_generate_gpu.py, test_lora_gpu.py and test_wav2vec2_gpu.py.
WHOLE_MODEL = {
    "uvx_encoder_fwd", "uvx_encoder_fwd_train", "uvx_encoder_bwd",
    "uvx_projector_fwd", "uvx_projector_bwd",
    "uvx_wav2vec2_frames", "uvx_wav2vec2_fwd", "uvx_wav2vec2_fwd_train", "uvx_wav2vec2_bwd",
    "uvx_llm_fwd", "uvx_llm_bwd", "uvx_llm_fwd_train", "uvx_llm_bwd_train", "uvx_llm_bwd_train_from",
    "uvx_llm_kl_loss", "uvx_llm_fwd_lora", "uvx_llm_bwd_lora",
    "uvx_llm_fwd_rows", "uvx_llm_kl_loss_rows", "uvx_llm_bwd_rows", "uvx_llm_bwd_rows_from",
    "uvx_llm_prefill", "uvx_llm_decode", "uvx_llm_prefill_chunk", "uvx_llm_prefill_chunk_logits",
}


def _dtype_entry_points():
    src = open(os.path.join(ROOT, "include", "uvx.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    names = set()
    for m in re.finditer(r"\bint32_t\s+(uvx_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        args = m.group(2)
        if re.search(r"\bint32_t\s+dtype\b", args) or re.search(r"\b(uvx_config_t|uvx_w2v_config_t)\s*\*\s*cfg\b", args):
            names.add(m.group(1))
    return names


def test_the_header_parse_finds_the_known_entry_points():
    names = _dtype_entry_points()
    for n in ("uvx_gemm", "uvx_rmsnorm_bwd", "uvx_attention_bwd", "uvx_ce_loss", "uvx_greedy_select", "uvx_embed_merge",
              "uvx_llm_fwd"):
        assert n in names, n
    assert "uvx_adamw_clip_step" not in names and "uvx_set_option" not in names
    assert WHOLE_MODEL <= names, WHOLE_MODEL - names        # the allow-list names only real entry points


def test_every_dtype_entry_point_has_an_f32_kernel_test():
    tests = open(os.path.join(ROOT, "tests", "test_f32_kernels_gpu.py")).read()
    missing = sorted(n for n in _dtype_entry_points() - WHOLE_MODEL if not re.search(rf"\b{n}\b", tests))
    assert not missing, f"no f32 test in tests/test_f32_kernels_gpu.py names {missing}"
