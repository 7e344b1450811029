"""A/B of the device sampler (uvx_sample_select) against the torch sampling path, on the GPU; writes the table of profiles/sample_select_ab.txt.

  python tools/sample_select_ab.py OUT.txt [--skip-generate]

(a) one call on the same bf16 logits [B, 128256]: uvx_sample_select (warpers + draw + bookkeeping, one launch) against UltravoxModel._sample
    (topk / sort / softmax / cumsum / scatter / multinomial; the loop's where / isin / any bookkeeping is NOT in this number).  Device events around
    blocks of 50 calls, the two versions alternating, 5 rounds each = 250 timed calls; median [min .. max] of the rounds' per-call means.
(b) ms per decoded token of generate(do_sample=True, temperature=0.6, top_p=0.9, max_new_tokens=64, eos_token_id=-1) at the 8B inference shape of
    `bench.py --workload c4s` (its config, imported), B = 1: torch.Generator against PhiloxGenerator, next to greedy.  As bench.py does it:
    (whole call - a max_new_tokens=1 call) / 63, host clock around a device synchronise, the three versions alternating over 4 rounds.
"""
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return f"{statistics.median(v):9.1f} [{min(v):8.1f} .. {max(v):8.1f}]"


def kernel_ab(lines):
    from ultravox_amd import ops
    from ultravox_amd.model import UltravoxModel
    V, block, rounds = 128256, 50, 5
    lines.append(f"(a) one call, bf16 logits [B, {V}] = 3 * randn (seed 0); us per call: median [min .. max] over {rounds} rounds of {block} calls, alternating")
    lines.append(f"{'B':>3} {'setting':<28} {'uvx_sample_select':>32} {'UltravoxModel._sample (torch)':>32}  ratio of medians")
    gen = torch.Generator(device="cuda").manual_seed(0)
    for B in (1, 8, 32):
        logits = (3.0 * torch.randn(B, V, device="cuda", generator=gen)).bfloat16()
        live = torch.ones(B, device="cuda", dtype=torch.int32)
        seq = torch.zeros(B, 1, device="cuda", dtype=torch.int64)
        counter = torch.zeros(2, device="cuda", dtype=torch.int32)
        for name, kw in (("temperature 0.6, top_p 0.9", dict(temperature=0.6, top_k=0, top_p=0.9)), ("top_k 50, top_p 0.95", dict(temperature=1.0, top_k=50, top_p=0.95))):
            calls = {"dev": lambda i: ops.sample_select(logits, seed=1, offset=i, unfinished=live, sequences=seq, counter=counter, **kw),
                     "torch": lambda i: UltravoxModel._sample(logits, kw["temperature"], kw["top_k"] or None, kw["top_p"], gen)}
            times = {k: [] for k in calls}
            for f in calls.values():
                for i in range(20):
                    f(i)
            for _ in range(rounds):
                for k, f in calls.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    a.record()
                    for i in range(block):
                        f(i)
                    b.record()
                    torch.cuda.synchronize()
                    times[k].append(a.elapsed_time(b) * 1e3 / block)
            lines.append(f"{B:>3} {name:<28} {spread(times['dev']):>32} {spread(times['torch']):>32}  {statistics.median(times['torch']) / statistics.median(times['dev']):6.2f}x")


def generate_ab(lines):
    import bench
    from ultravox_amd.config import UltravoxConfig
    from ultravox_amd.frontend import WhisperFeatureExtractor
    from ultravox_amd.generation import PhiloxGenerator
    from ultravox_amd.model import UltravoxModel
    from ultravox_amd.synthetic import synthetic_batch
    wl = bench.WORKLOADS["c4s"]
    cfg = UltravoxConfig(audio_model_id=wl["audio"], text_model_id=wl["text"], hidden_size=4096, stack_factor=8, projector_ln_mid=True, torch_dtype="bfloat16")
    model = UltravoxModel(cfg, device="cuda", dtype=torch.bfloat16, seed=0, rope_len=1024, with_backward=False, consume_state_dict=True)
    fe = WhisperFeatureExtractor(cfg.audio_config.num_mel_bins, device="cuda")
    batch = synthetic_batch(cfg, 1, wl["seconds"], n_text=128, audio_start=16, n_supervised=32, rank=0)
    pcm = batch.pop("pcm").to("cuda")
    batch.pop("labels")
    gb = {k: v.to("cuda") for k, v in batch.items()}
    N, rounds = 64, 4
    sample = dict(do_sample=True, temperature=0.6, top_p=0.9)
    tg, pg = torch.Generator(device="cuda").manual_seed(0), PhiloxGenerator(0)
    variants = {"greedy (uvx_greedy_select)": {}, "sampling, torch.Generator": dict(generator=tg, **sample), "sampling, PhiloxGenerator": dict(generator=pg, **sample)}

    def timed(n, kw, reps=2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            model.generate(audio_values=fe.logmel_device(pcm), max_new_tokens=n, eos_token_id=-1, **gb, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps
    for kw in variants.values():
        timed(N, kw, 1)
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, kw in variants.items():
            ms[k].append((timed(N, kw) - timed(1, kw)) / (N - 1) * 1e3)
    lines.append("")
    lines.append(f"(b) generate() at the 8B shape of bench.py --workload c4s, B = 1, {N} new tokens; ms per decoded token: median [min .. max] over {rounds} rounds, alternating")
    for k, v in ms.items():
        lines.append(f"    {k:<28} {statistics.median(v):7.3f} [{min(v):7.3f} .. {max(v):7.3f}]")


def main():
    out = sys.argv[1]
    lines = ["# uvx_sample_select against the torch sampling path (tools/sample_select_ab.py; MI355X, one process, one call)"]
    kernel_ab(lines)
    if "--skip-generate" not in sys.argv:
        generate_ab(lines)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
