"""Records tests/golden/pipeline_preprocess_reference.json: the REFERENCE UltravoxPipeline.preprocess (ultravox_pipeline.py:55-95) on the cases of
`cases()` below, over the reference's own UltravoxProcessor with the HF WhisperFeatureExtractor and tests/fake_tokenizer.FakeChatTokenizer, as
make_golden.py sets them up.  Run where a snapshot of the reference is at hand:

    python tests/golden/make_pipeline_golden.py PATH_TO_REFERENCE

The fixture travels, the reference does not; tests/test_sample_penalized_cpu.py replays `cases()` through ultravox_amd.pipeline and compares."""
import json
import logging
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "pipeline_preprocess_reference.json")
AUDIO_STRIDE = 97


def cases():
    """name -> the pipeline's input dict (built anew on every call: preprocess appends to `turns`)."""
    pcm = lambda n, seed: np.random.RandomState(seed).randn(n) * 0.1
    sys_turn = {"role": "system", "content": "Be brief ."}
    return {
        "audio_only_f32": {"audio": pcm(16000, 1).astype(np.float32), "sampling_rate": 16000},
        "audio_f64_no_rate": {"audio": pcm(8000, 2)},
        "audio_i16_system_turn": {"audio": (pcm(24000, 3) * 32768).astype(np.int16), "turns": [dict(sys_turn)], "sampling_rate": 16000},
        "audio_i32_prompt": {"audio": (pcm(12000, 4) * 2147483648).astype(np.int32), "prompt": "Transcribe <|audio|> please", "sampling_rate": 16000},
        "prompt_without_placeholder": {"audio": pcm(16000, 5).astype(np.float32), "prompt": "What is said ?", "turns": [], "sampling_rate": 16000},
        "last_turn_is_the_users": {"audio": pcm(16000, 6).astype(np.float32), "sampling_rate": 16000,
                                   "turns": [dict(sys_turn), {"role": "user", "content": "Listen to <|audio|> and answer"}]},
        "after_an_assistant_turn": {"audio": pcm(40000, 7).astype(np.float32), "sampling_rate": 16000,
                                    "turns": [{"role": "user", "content": "Hello"}, {"role": "assistant", "content": "Hi there"}]},
        "text_only": {"turns": [dict(sys_turn), {"role": "user", "content": "What is two plus two ?"}]},
        "long_audio": {"audio": pcm(16000 * 35, 8).astype(np.float32), "sampling_rate": 16000},
    }


class Warnings(logging.Handler):
    """Collects the messages logged at WARNING on the root logger while it is installed."""

    def __init__(self):
        super().__init__(logging.WARNING)
        self.messages = []

    def emit(self, record):
        self.messages.append(record.getMessage())

    def __enter__(self):
        logging.getLogger().addHandler(self)
        return self

    def __exit__(self, *a):
        logging.getLogger().removeHandler(self)


def record(preprocess, inputs):
    """-> what one preprocess call returned and did, as JSON: integer outputs with dtype and shape, audio_values' dtype, shape and every
    AUDIO_STRIDE-th value, the turns the caller's list holds afterwards, the warnings."""
    with Warnings() as w:
        out = preprocess(inputs)
    got = {}
    for k in out.keys():
        v = torch.as_tensor(out[k])
        got[k] = {"dtype": str(v.dtype), "shape": list(v.shape)}
        if k != "audio_values":
            got[k]["values"] = v.tolist()
        else:                   # every AUDIO_STRIDE-th element: enough to tell a wrong conversion or a wrong sampling rate, small enough to commit
            got[k]["sampled"] = v.flatten()[::AUDIO_STRIDE].tolist()
    return {"out": got, "turns": inputs.get("turns"), "warnings": w.messages}


def main(reference):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, reference)
    import peft_stub
    peft_stub.install()
    import transformers
    from fake_tokenizer import FakeChatTokenizer
    from ultravox.model import ultravox_pipeline, ultravox_processing
    fe = transformers.WhisperFeatureExtractor()
    ap = type("AP", (), {"feature_extractor": fe, "model_input_names": fe.model_input_names, "__call__": staticmethod(lambda *a, **k: fe(*a, **k))})()
    tok = FakeChatTokenizer()
    tok.pad_token_id = tok.eos_token_id
    proc = ultravox_processing.UltravoxProcessor.__new__(ultravox_processing.UltravoxProcessor)      # (past ProcessorMixin.__init__'s type checks)
    proc.audio_padding, proc.encoder_ds_factor, proc.stack_factor = "longest", 2, 8
    proc.audio_placeholder, proc.audio_context_size = "<|audio|>", 3000
    proc.vocab, proc.audio_token_replacement = tok.get_vocab(), tok.eos_token
    proc.audio_processor, proc.tokenizer = ap, tok
    pipe = ultravox_pipeline.UltravoxPipeline.__new__(ultravox_pipeline.UltravoxPipeline)              # (no model to load: preprocess reads two fields)
    pipe.processor, pipe.model = proc, types.SimpleNamespace(dtype=torch.float32)
    got = {name: record(pipe.preprocess, inputs) for name, inputs in cases().items()}
    with open(OUT, "w") as f:
        json.dump(got, f, indent=1)
    print(OUT, {k: v["out"]["input_ids"]["shape"] for k, v in got.items()})


if __name__ == "__main__":
    main(sys.argv[1])
