"""A/B of sampling under a repetition penalty on the device (uvx_sample_select_penalized) against the torch path it replaces, on the GPU; writes the
table of profiles/sample_select_penalized_ab.txt.

  python tools/sample_select_penalized_ab.py OUT.txt [--skip-generate]

(a) one call on the same bf16 logits [B, 128256] with a 512-token row of seen ids, temperature 0.6 + top_p 0.9 + penalty 1.1:
    uvx_sample_select_penalized (penalty + warpers + draw + bookkeeping, one launch) against what the generic loop runs for the same decision -
    logits.float(), generation.repetition_penalty_ (gather / where / scatter_) and UltravoxModel._sample (topk / sort / softmax / cumsum / scatter /
    multinomial; the loop's cat / where / isin / any bookkeeping is NOT in that number) - and, next to them, uvx_sample_select on the same logits,
    which shows what the penalty costs.  Both entry points are called bare, on buffers made once.  Device events around blocks of 50 calls, the
    versions alternating, 5 rounds each = 250 timed calls; median [min .. max] of the rounds' per-call means.  (Every call of the new entry point
    sets one more bit of the bitmap: a few hundred bits of 128256 by the end.)
(b) ms per decoded token of generate(max_new_tokens=64, eos_token_id=-1) at the 8B inference shape of `bench.py --workload c4s` (its config,
    imported), B = 1, sampling at temperature 0.6 + top_p 0.9: torch.Generator + penalty 1.1, PhiloxGenerator(penalty_on_device=True) + penalty 1.1,
    PhiloxGenerator without a penalty, and greedy + penalty 1.1.  As bench.py does it: (whole call - a max_new_tokens=1 call) / 63, host clock
    around a device synchronise, the versions alternating over 4 rounds.
"""
import ctypes as C
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return f"{statistics.median(v):9.1f} [{min(v):8.1f} .. {max(v):8.1f}]"


def apart(slow, fast):
    return "min of the slower side's rounds above the max of the faster side's" if min(slow) > max(fast) else "the rounds OVERLAP"


def verdict(torch_side, dev_side):
    if statistics.median(torch_side) > statistics.median(dev_side):
        return apart(torch_side, dev_side)
    return "the TORCH side is faster: " + apart(dev_side, torch_side)


def kernel_ab(lines):
    from ultravox_amd import _lib, generation, ops
    from ultravox_amd._lib import check, ptr, stream_ptr
    from ultravox_amd.model import UltravoxModel
    V, block, rounds, n_seen, penalty, t, top_p = 128256, 50, 5, 512, 1.1, 0.6, 0.9
    lines.append(f"(a) one call, bf16 logits [B, {V}] = 3 * randn (seed 0), {n_seen} seen ids per row, temperature {t}, top_p {top_p}, penalty {penalty}; us per call: "
                 f"median [min .. max] over {rounds} rounds of {block} calls, alternating")
    lines.append(f"{'B':>3} {'uvx_sample_select_penalized':>32} {'float + repetition_penalty_ + _sample':>38} {'uvx_sample_select':>32}  torch / device   device / unpenalised")
    gen = torch.Generator(device="cuda").manual_seed(0)
    lib = _lib.lib()
    for B in (1, 8, 32):
        logits = (3.0 * torch.randn(B, V, device="cuda", generator=gen)).bfloat16()
        ids = torch.randint(0, V, (B, n_seen), device="cuda", generator=gen)
        seen = ops.seen_mark(ids, V)
        live = torch.ones(B, device="cuda", dtype=torch.int32)
        seq = torch.zeros(B, 1, device="cuda", dtype=torch.int64)
        nxt = torch.empty(B, device="cuda", dtype=torch.int64)
        counter = torch.zeros(2, device="cuda", dtype=torch.int32)
        book = lambda i: (None, 0, 0, ptr(live), ptr(nxt), ptr(seq), 1, 0, None, None, i, ptr(counter))

        def dev(i):
            check(lib.uvx_sample_select_penalized(stream_ptr(), _lib.BF16, ptr(logits), B, V, penalty, ptr(seen), seen.shape[1], t, 0, top_p, 0.0, 1, 1, i,
                                                  None, None, *book(i)), "uvx_sample_select_penalized")

        def plain(i):
            check(lib.uvx_sample_select(stream_ptr(), _lib.BF16, ptr(logits), B, V, t, 0, top_p, 0.0, 1, 1, i, None, None, *book(i)), "uvx_sample_select")
        calls = {"dev": dev,
                 "torch": lambda i: UltravoxModel._sample(generation.repetition_penalty_(logits.float(), ids, penalty), t, None, top_p, gen),
                 "plain": plain}
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
        med = {k: statistics.median(v) for k, v in times.items()}
        lines.append(f"{B:>3} {spread(times['dev']):>32} {spread(times['torch']):>38} {spread(times['plain']):>32}  {med['torch'] / med['dev']:6.2f}x"
                     f"         {med['dev'] / med['plain']:6.2f}x   ({verdict(times['torch'], times['dev'])})")


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
    TORCH, DEV = "sampling + penalty 1.1, torch.Generator", "sampling + penalty 1.1, PhiloxGenerator(penalty_on_device)"
    variants = {TORCH: dict(generator=torch.Generator(device="cuda").manual_seed(0), repetition_penalty=1.1, **sample),
                DEV: dict(generator=PhiloxGenerator(0, penalty_on_device=True), repetition_penalty=1.1, **sample),
                "sampling, PhiloxGenerator, no penalty": dict(generator=PhiloxGenerator(0), **sample),
                "greedy + penalty 1.1": dict(repetition_penalty=1.1)}

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
        lines.append(f"    {k:<60} {statistics.median(v):7.3f} [{min(v):7.3f} .. {max(v):7.3f}]")
    lines.append(f"    device against torch under the penalty: {verdict(ms[TORCH], ms[DEV])}")


def main():
    out = sys.argv[1]
    lines = ["# uvx_sample_select_penalized against the torch path of sampling under a repetition penalty (tools/sample_select_penalized_ab.py; MI355X, one process, one call)"]
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
