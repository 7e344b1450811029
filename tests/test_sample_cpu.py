"""The device sampler's reference, random numbers and host logic, without a GPU: tests/sample_util.py against [3P] HF's own warpers, the numpy
Philox against a second restatement and a uniformity test, PhiloxGenerator's bookkeeping, and generate()'s PhiloxGenerator branch on the simulated
device of tests/test_generate_host_cpu.py (the kernel itself: tests/test_sample_gpu.py)."""
import itertools
import types

import numpy as np
import pytest
import torch

import sample_util as SU
import ultravox_amd.model as M
from test_generate_host_cpu import D, V, FakeLib, left_padded
from ultravox_amd import _lib
from ultravox_amd.generation import PhiloxGenerator
from ultravox_amd.model import KVState, UltravoxModel


def grid(Vv):
    return itertools.product((1.0, 0.7), (0, 1, 5, Vv, Vv + 3), (1.0, 0.9, 1e-6), (0.0, 0.1), (1, 3))


@pytest.mark.parametrize("Vv", [5, 1025])
def test_reference_keeps_what_hf_warpers_keep(Vv):
    """RowRef's kept set == that of TemperatureLogitsWarper -> TopKLogitsWarper -> TopPLogitsWarper -> MinPLogitsWarper from the installed
    transformers, on tie-free random rows, over the whole parameter grid of the GPU test."""
    from transformers.generation import logits_process as LP
    g = np.random.default_rng(Vv)
    n = 0
    for row in range(3):
        logits = (g.standard_normal(Vv) * 3).astype(np.float32)
        assert len(np.unique(logits)) == Vv
        refs = {t: SU.RowRef(SU.x_of(logits, t)) for t in (1.0, 0.7)}
        for t, k, p, mp, keep in grid(Vv):
            s = torch.from_numpy(logits)[None].clone()
            if t != 1.0:
                s = LP.TemperatureLogitsWarper(t)(None, s)
            if k > 0:
                s = LP.TopKLogitsWarper(k, min_tokens_to_keep=keep)(None, s)
            if p < 1.0:
                s = LP.TopPLogitsWarper(p, min_tokens_to_keep=keep)(None, s)
            if mp > 0.0:
                s = LP.MinPLogitsWarper(mp, min_tokens_to_keep=keep)(None, s)
            ref = refs[t].warp(k, p, mp, keep)
            if not SU.margins_ok(ref):          # (f32 HF against f64 at a boundary closer than f32 resolves: not a statement about either)
                continue
            n += 1
            assert np.array_equal(ref["kept"], torch.isfinite(s[0]).numpy()), (row, t, k, p, mp, keep)
            want = torch.softmax(s[0].double(), -1).numpy()
            assert np.allclose(ref["probs"], want, rtol=1e-5, atol=0)
    assert n > 300            # the margins hold almost everywhere on such rows


def test_reference_tie_and_infinity_rules():
    x = np.array([1.0, 3.0, 3.0, -np.inf, 0.5, 3.0], dtype=np.float32)
    r = SU.RowRef(x)
    assert r.warp(top_k=1)["kept"].tolist() == [False, True, True, False, False, True]          # ties with the k-th value stay
    assert r.warp(top_p=1e-6)["kept"].tolist() == [False, True, True, False, False, True]       # an equal group stays or goes together
    assert r.warp()["kept"].tolist() == [True, True, True, False, True, True]
    none = SU.RowRef(np.full(4, -np.inf, dtype=np.float32)).warp(top_k=2, top_p=0.5, min_p=0.1)
    assert not none["kept"].any() and SU.token_ok(0, 0.3, none) and not SU.token_ok(1, 0.3, none)
    ref = SU.RowRef(np.log(np.array([0.1, 0.2, 0.3, 0.4], dtype=np.float32))).warp()
    assert [SU.token_ok(t, 0.25, ref) for t in range(4)] == [False, True, False, False]
    assert SU.token_ok(0, 0.0, ref) and SU.token_ok(3, 1 - 2.0 ** -24, ref) and not SU.token_ok(2, 1 - 2.0 ** -24, ref)


def test_numpy_philox_against_plain_integers_and_uniformity():
    g = np.random.default_rng(7)
    key = g.integers(0, 2 ** 32, size=(1000, 2), dtype=np.uint64).astype(np.uint32)
    ctr = g.integers(0, 2 ** 32, size=(1000, 4), dtype=np.uint64).astype(np.uint32)
    got = SU.philox4x32_10(key, ctr)
    for i in range(1000):
        assert tuple(int(v) for v in got[i]) == SU.philox_python(tuple(map(int, key[i])), tuple(map(int, ctr[i]))), i
    # the known-answer vectors of the Random123 distribution (Philox4x32-10)
    assert SU.philox_python((0, 0), (0, 0, 0, 0)) == (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)
    assert SU.philox_python((0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF,) * 4) == (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)
    u = SU.philox_uniform(seed=(5 << 32) | 11, offset=(1 << 32) + 3, B=4096)
    assert u.min() >= 0.0 and u.max() < 1.0
    counts = np.bincount((u * 8).astype(int), minlength=8)
    chi2 = float(((counts - 512.0) ** 2 / 512.0).sum())
    assert chi2 < SU.chi2_quantile(7, 1e-6), (chi2, counts)
    assert 39.0 < SU.chi2_quantile(7, 1e-6) < 45.0          # (scipy: 41.5; Wilson-Hilferty: 40.6)


def test_philox_generator_bookkeeping():
    g = PhiloxGenerator(5)
    assert (g.seed, g.offset) == (5, 0)
    assert g.advance(3) is g and g.offset == 3 and g.advance(0).offset == 3
    g.advance(2 ** 40)
    assert g.offset == 3 + 2 ** 40 and g.seed == 5
    assert g.manual_seed(2 ** 63 + 1) is g and (g.seed, g.offset) == (2 ** 63 + 1, 0)       # a new seed starts its stream over
    g.advance(2 ** 64 - 1).advance(2)
    assert g.offset == 1                                     # the counter's 64 bits wrap
    with pytest.raises(ValueError):
        g.advance(-1)
    assert PhiloxGenerator().seed == 0


class SamplingFakeLib(FakeLib):
    """FakeLib plus a stand-in for uvx_sample_select that records its sampling arguments and picks the arg-max (include/uvx.h for the rest)."""

    def uvx_sample_select(self, st, code, logits, B, Vv, temperature, top_k, top_p, min_p, min_keep, seed, offset, uniforms, probs, *book):
        self.calls.append(("sample", dict(temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p, min_keep=min_keep, seed=seed, offset=offset)))
        assert uniforms is None and probs is None
        return self.uvx_greedy_select(st, code, logits, B, Vv, *book)


@pytest.fixture()
def model(monkeypatch):
    fake = SamplingFakeLib()
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    monkeypatch.setattr(M, "ptr", lambda t: t)
    monkeypatch.setattr(M, "stream_ptr", lambda: None)
    monkeypatch.setattr(M, "check", lambda rc, what="": None)
    monkeypatch.setattr(M.C, "byref", lambda x: x)
    monkeypatch.setattr(M.C, "c_size_t", lambda x: x)
    m = UltravoxModel.__new__(UltravoxModel)
    m.device, m.dtype, m.code, m.text_lora_r = torch.device("cpu"), torch.float32, 0, 0
    m.config = types.SimpleNamespace(vocab_size=V, text_config=types.SimpleNamespace(eos_token_id=2, hidden_size=D))
    table = (torch.arange(V, dtype=torch.float32)[:, None] + 1.0).repeat(1, D)
    m._llm = {"rope_len": 4096, "embed": table}
    m._c = types.SimpleNamespace(llm_layers=1)
    m._lw, m._ws = None, {}
    m._embed_merge = lambda emb, ids, *a: table[ids]
    m.fake = fake
    return m


def test_generate_under_a_philox_generator_host_loop(model):
    """One uvx_sample_select per token with offset = the generator's offset + step, HF's defaults for what is not given, the generator advanced by
    the steps run, the same KV state as the greedy loop - and no such call without a PhiloxGenerator."""
    ids, am = left_padded(2, 9, [0, 3])
    gen = PhiloxGenerator(77).advance(10)
    out = model.generate(ids, attention_mask=am, max_new_tokens=5, eos_token_id=-1, do_sample=True, temperature=0.6, top_p=0.9, generator=gen,
                         return_dict_in_generate=True)
    calls = [c[1] for c in model.fake.calls if c[0] == "sample"]
    assert [c["offset"] for c in calls] == [10, 11, 12, 13, 14] and gen.offset == 15 and {c["seed"] for c in calls} == {77}
    assert all(abs(c["temperature"] - 0.6) < 1e-7 and c["top_k"] == 0 and abs(c["top_p"] - 0.9) < 1e-7 and c["min_p"] == 0.0 and c["min_keep"] == 1
               for c in calls)
    greedy = model.generate(ids, attention_mask=am, max_new_tokens=5, eos_token_id=-1, return_dict_in_generate=True)
    assert torch.equal(out.sequences, greedy.sequences)      # (the stand-in picks the arg-max)
    st, sg = out.past_key_values, greedy.past_key_values
    assert isinstance(st, KVState) and (st.cur_len, st.Tmax) == (sg.cur_len, sg.Tmax) == (13, 14) and torch.equal(st.pos_next, sg.pos_next)
    # an early stop: fewer steps run, the offset follows them
    stop = int(out.sequences[0, 9 + 1])
    early = model.generate(ids[:1], max_new_tokens=5, eos_token_id=stop, do_sample=True, top_k=3, min_p=0.05, generator=gen)
    n = early.shape[1] - 9
    assert n < 5 and gen.offset == 15 + n
    assert [c[1] for c in model.fake.calls if c[0] == "sample"][-1]["top_k"] == 3
    # torch's sampler and greedy decoding never reach the new entry point
    model.fake.calls.clear()
    model.generate(ids, attention_mask=am, max_new_tokens=3, eos_token_id=-1, do_sample=True, top_k=5, generator=torch.Generator().manual_seed(0))
    model.generate(ids, attention_mask=am, max_new_tokens=3, eos_token_id=-1, do_sample=True, top_k=5)
    model.generate(ids, attention_mask=am, max_new_tokens=3, eos_token_id=-1, generator=gen)          # greedy: the generator is not consulted
    assert not [c for c in model.fake.calls if c[0] == "sample"] and gen.offset == 15 + n


@pytest.mark.parametrize("kw, name", [(dict(repetition_penalty=1.3), "score processors"), (dict(no_repeat_ngram_size=2), "score processors"),
                                      (dict(logits_processor=[lambda i, s: s]), "score processors"),
                                      (dict(stopping_criteria=[lambda i, s: False]), "stopping_criteria"),
                                      (dict(output_logits=True, return_dict_in_generate=True), "output_logits"), (dict(num_beams=2), "num_beams")])
def test_philox_generator_refuses_what_the_kernel_does_not_do(model, kw, name):
    ids, am = left_padded(2, 7, [0, 2], seed=5)
    gen = PhiloxGenerator(1)
    with pytest.raises(ValueError, match=f"PhiloxGenerator.*{name}"):
        model.generate(ids, attention_mask=am, max_new_tokens=3, eos_token_id=-1, do_sample=True, generator=gen, **kw)
    assert gen.offset == 0 and not model.fake.calls
    model.generate(ids, attention_mask=am, max_new_tokens=3, eos_token_id=-1, do_sample=True, generator=torch.Generator().manual_seed(0), **kw)    # the torch path takes them


def test_local_inference_owns_one_philox_stream():
    from fake_tokenizer import FakeChatTokenizer
    from oracle.reference_cpu import FeatureExtractorRef
    from ultravox_amd.inference import LocalInference, VoiceSample
    from ultravox_amd.processing import UltravoxProcessor
    tok = FakeChatTokenizer()
    seen = []

    class Stub:
        device, dtype = torch.device("cpu"), torch.float32

        def generate(self, **kw):
            seen.append(kw)
            return torch.cat([kw["input_ids"], torch.tensor([[128009]])], 1)
    proc = UltravoxProcessor(FeatureExtractorRef(80), tokenizer=tok)
    inf = LocalInference(Stub(), proc, tok, dtype=torch.float32, sampler_seed=9)
    inf.infer(VoiceSample.from_prompt("Hi"), temperature=0.6)
    inf.infer(VoiceSample.from_prompt("Hi"), temperature=0.6)
    inf.infer(VoiceSample.from_prompt("Hi"))
    assert isinstance(seen[0]["generator"], PhiloxGenerator) and seen[0]["generator"] is seen[1]["generator"] is inf.sampler and inf.sampler.seed == 9
    assert seen[0]["do_sample"] and "generator" not in seen[2] and not seen[2]["do_sample"]           # temperature 0 / None: greedy, as before
    seen.clear()
    LocalInference(Stub(), proc, tok, dtype=torch.float32).infer(VoiceSample.from_prompt("Hi"), temperature=0.6)
    assert "generator" not in seen[0] and seen[0]["do_sample"]                                        # the default keeps torch's sampler


def test_the_select_kernels_have_no_scratch_segment():
    """hipcc's kernel-resource-usage remarks for select.hip with the package's own flags: the eight instantiations of the select kernel (reader x
    chooser x dtype), the mark kernel and both instantiations of the argmax kernel, no scratch."""
    import re
    import subprocess

    from ultravox_amd import build as B
    src = B.CSRC / "select.hip"
    cmd = [B._hipcc(), *B.FLAGS, *B.EXTRA_FLAGS.get(src.name, []), "-Rpass-analysis=kernel-resource-usage", "--cuda-device-only", "-c", str(src), "-o", "/dev/null"]
    err = subprocess.run(cmd, capture_output=True, text=True).stderr
    names = re.findall(r"Function Name: (\S+)", err)
    scratch = [int(x) for x in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", err)]
    assert len(names) == len(scratch) == 11, names
    count = lambda kernel: sum(kernel in n for n in names)
    assert (count("select_k"), count("seen_mark_k"), count("argmax_k")) == (8, 1, 2) and len(set(names)) == 11, names
    assert scratch == [0] * 11, list(zip(names, scratch))
