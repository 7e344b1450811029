"""Differential tests against the REFERENCE processor, data-proc and collator: hypothesis drew audio counts / lengths / prompt shapes
(tests/golden/make_golden.py::live_reference_cases, same strategies and example counts), the reference's outputs for every drawn case
are recorded in tests/golden/live_reference.json, and the mirror must reproduce them: every integer output and dtype exactly, the
audio tensor's shape, and its values to 2e-4 against the HF WhisperFeatureExtractor chunks the reference stacked."""
import json
import os
import types

import numpy as np
import pytest
import torch

from fake_tokenizer import FakeTokenizer
from oracle.reference_cpu import FeatureExtractorRef
from ultravox_amd.processing import UltravoxProcessor

pytestmark = pytest.mark.filterwarnings("ignore::DeprecationWarning")


@pytest.fixture(scope="module")
def cases(golden_dir):
    with open(os.path.join(golden_dir, "live_reference.json")) as f:
        return json.load(f)


def assert_tensor(got, want, what):
    g = torch.as_tensor(got)
    assert str(g.dtype) == want["dtype"] and list(g.shape) == want["shape"] and g.tolist() == want["values"], what


def reference_audio_values(audios, want):
    """The reference's audio_values, rebuilt from its recorded chunk table: the HF WhisperFeatureExtractor call it makes (audio
    padded to two hops, padding="longest", pad_to_multiple_of=hop), sliced into 3000-frame chunks and right-padded to one width."""
    import transformers
    hop = 160
    feats = transformers.WhisperFeatureExtractor()([np.pad(a, (0, 2 * hop - len(a))) if len(a) < 2 * hop else a for a in audios],
                                                  sampling_rate=16000, padding="longest", pad_to_multiple_of=hop, truncation=False,
                                                  return_attention_mask=True)
    hf = torch.as_tensor(feats.input_features)
    width = want["shape"][-1]
    return torch.stack([torch.nn.functional.pad(hf[i, :, off:off + 3000], (0, width - hf[i, :, off:off + 3000].shape[-1]))
                        for i, off in want["chunks"]])


def test_processor_agrees_with_the_live_reference(cases):
    tok = FakeTokenizer()
    tok.pad_token_id = tok.eos_token_id
    mine = UltravoxProcessor(FeatureExtractorRef(80), tokenizer=tok)
    assert len(cases["processor"]) == 30
    for case in cases["processor"]:
        lengths, words = case["lengths"], case["words"]
        rng = np.random.RandomState(case["seed"])
        audios = [rng.randn(n).astype(np.float32) * 0.1 for n in lengths]
        n_ph = max(0, len(audios) + case["placeholder_delta"])            # sometimes one placeholder too few / too many
        parts = [" ".join(words[i::n_ph + 1]) or "x" for i in range(n_ph + 1)]
        text = " <|audio|> ".join(parts)
        kw = dict(audios=audios, sampling_rate=16000, include_audio_num_chunks=case["chunks"]) if audios else {}
        try:
            got, got_err = mine(text, **kw), None
        except ValueError as e:
            got, got_err = None, str(e)
        assert got_err == case.get("error"), (text, lengths)
        if got is None:
            continue
        want = case["want"]
        assert set(got.keys()) == set(want.keys()), (sorted(got.keys()), sorted(want.keys()))
        for k in want:
            if k == "audio_values":
                g, w = torch.as_tensor(got[k]), want[k]
                assert list(g.shape) == w["shape"] and str(g.dtype) == w["dtype"]
                ref = reference_audio_values(audios, w)
                assert torch.allclose(g, ref, atol=2e-4), (g - ref).abs().max()
            else:
                assert_tensor(got[k], want[k], (k, text, lengths))


def test_dataproc_agrees_with_the_live_reference(cases):
    from fake_tokenizer import FakeChatTokenizer
    from ultravox_amd.config import LossMaskType
    from ultravox_amd.data_proc import UltravoxDataproc
    assert len(cases["dataproc"]) == 40
    for case in cases["dataproc"]:
        n_samples = case["n_samples"]
        user = " ".join(case["words"]) + (" <|audio|>" if n_samples is not None else "") + (" thanks" if case["tail"] else "")
        messages = ([{"role": "system", "content": "Be brief ."}] if case["system"] else []) + \
            [{"role": "user", "content": user}, {"role": "assistant", "content": " ".join(case["reply"])}]
        audio = None if n_samples is None else np.random.RandomState(1).randn(n_samples).astype(np.float32) * 0.1
        kw = dict(inference_mode=case["inference_mode"], include_alt_fields=case["include_alt_fields"],
                  max_response_tokens=case["max_response_tokens"])
        tok_m = FakeChatTokenizer("right")
        tok_m.pad_token_id = tok_m.eos_token_id
        mine = UltravoxDataproc([], UltravoxProcessor(FeatureExtractorRef(80), tokenizer=tok_m), LossMaskType(case["mask"]), **kw)
        try:
            got, got_err = mine._process(types.SimpleNamespace(messages=[dict(m) for m in messages], audio=audio, sample_rate=16000,
                                                               audio_transcript=case["transcript"])), None
        except (ValueError, IndexError) as e:
            got, got_err = None, [type(e).__name__, str(e)]
        assert got_err == case.get("error"), (messages, case["mask"], kw)
        if got is None:
            continue
        want = case["want"]
        assert set(got) == set(want)
        for k in want:
            if k == "audio_values":
                assert list(got[k].shape) == want[k]["shape"]
                continue
            g = got[k].tolist() if hasattr(got[k], "tolist") else got[k]
            assert g == want[k]["value"], (k, messages, case["mask"], kw)


def test_collator_agrees_with_the_live_reference(cases):
    """DataCollatorForSeq2SeqWithAudio over data-proc features: the reference's own __call__ body ran with the [3P]
    DataCollatorForSeq2Seq padding it inherits stubbed by the same rule (pad ids / mask / labels on tokenizer.padding_side),
    including the alt fields of the KL path and the left-padding displacement of audio_token_start_idx."""
    import torch.nn.functional as F
    from fake_tokenizer import FakeChatTokenizer
    from ultravox_amd.config import LossMaskType
    from ultravox_amd.data_proc import UltravoxDataproc
    from ultravox_amd.processing import DataCollatorForSeq2SeqWithAudio
    assert len(cases["collator"]) == 25
    for case in cases["collator"]:
        side, alt, picks = case["side"], case["alt"], case["picks"]
        tok = FakeChatTokenizer(side)
        tok.pad_token_id = tok.eos_token_id
        dp = UltravoxDataproc([], UltravoxProcessor(FeatureExtractorRef(80), tokenizer=tok), LossMaskType.LAST_ASSISTANT, include_alt_fields=alt)
        rng = np.random.RandomState(0)
        bank = {
            "asr": ([{"role": "user", "content": "Transcribe <|audio|>"}, {"role": "assistant", "content": "a b c"}], 16000, "a b c"),
            "qa": ([{"role": "user", "content": "Listen <|audio|> and answer now please"}, {"role": "assistant", "content": "ok then"}], 40000, "hm"),
            "long": ([{"role": "user", "content": "<|audio|>"}, {"role": "assistant", "content": "long one indeed yes"}], 500000, "x y"),
            "two": ([{"role": "system", "content": "sys"}, {"role": "user", "content": "A <|audio|> B"}, {"role": "assistant", "content": "r"}], 8000, None),
        }
        feats = []
        for name in picks:
            msgs, n, tr = bank[name]
            feats.append(dp._process(types.SimpleNamespace(messages=[dict(m) for m in msgs], audio=rng.randn(n).astype(np.float32) * 0.1,
                                                           sample_rate=16000, audio_transcript=tr)))
        audio = [x.clone() for f in feats for x in f.get("audio_values", [])]
        got = DataCollatorForSeq2SeqWithAudio(tok, include_alt_fields=alt)(feats)
        want = case["want"]
        assert set(got) == set(want), (sorted(got), sorted(want))
        for k in want:
            if k == "audio_values":          # the reference stacks the features right-padded to the longest (recorded: dtype and shape)
                w = want[k]
                assert str(got[k].dtype) == w["dtype"] and list(got[k].shape) == w["shape"], (side, alt, picks)
                assert torch.equal(got[k], torch.stack([F.pad(x, (0, w["shape"][-1] - x.shape[-1])) for x in audio])), (side, alt, picks)
            else:
                assert_tensor(got[k], want[k], (k, side, alt, picks))
