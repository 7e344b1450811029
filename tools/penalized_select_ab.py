"""A/B of greedy decoding under a repetition penalty on the device (uvx_greedy_select_penalized) against the host policy it replaces, on the GPU;
writes the table of profiles/penalized_select_ab.txt.

  python tools/penalized_select_ab.py OUT.txt [--skip-generate]

(a) one call on the same bf16 logits [B, 128256] with a 512-token row of seen ids: uvx_greedy_select_penalized (penalty + argmax + bookkeeping, one
    launch) against what the generic loop runs for the same decision - logits.float(), generation.repetition_penalty_ (gather / where / scatter_)
    and argmax; the loop's cat / where / isin / any bookkeeping is NOT in that number - and, next to them, uvx_greedy_select on the same logits.
    Device events around blocks of 50 calls, the versions alternating, 5 rounds each = 250 timed calls; median [min .. max] of the rounds'
    per-call means.
(b) ms per decoded token of generate(repetition_penalty=1.1, max_new_tokens=64, eos_token_id=-1) at the 8B inference shape of
    `bench.py --workload c4s` (its config, imported), B = 1: model.penalized_select on against off, next to plain greedy.  As bench.py does it:
    (whole call - a max_new_tokens=1 call) / 63, host clock around a device synchronise, the three versions alternating over 4 rounds.
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


def kernel_ab(lines):
    from ultravox_amd import _lib, generation, ops
    from ultravox_amd._lib import check, ptr, stream_ptr
    V, block, rounds, n_seen, penalty = 128256, 50, 5, 512, 1.1
    lines.append(f"(a) one call, bf16 logits [B, {V}] = 3 * randn (seed 0), {n_seen} seen ids per row, penalty {penalty}; us per call: median [min .. max] over "
                 f"{rounds} rounds of {block} calls, alternating")
    lines.append(f"{'B':>3} {'uvx_greedy_select_penalized':>32} {'float + repetition_penalty_ + argmax':>38} {'uvx_greedy_select':>32}  host / device   device / plain greedy")
    gen = torch.Generator(device="cuda").manual_seed(0)
    for B in (1, 8):
        logits = (3.0 * torch.randn(B, V, device="cuda", generator=gen)).bfloat16()
        ids = torch.randint(0, V, (B, n_seen), device="cuda", generator=gen)
        seen = ops.seen_mark(ids, V)
        live = torch.ones(B, device="cuda", dtype=torch.int32)
        seq = torch.zeros(B, 1, device="cuda", dtype=torch.int64)
        nxt = torch.empty(B, device="cuda", dtype=torch.int64)
        counter = torch.zeros(2, device="cuda", dtype=torch.int32)
        lib = _lib.lib()

        def plain(i):
            check(lib.uvx_greedy_select(stream_ptr(), _lib.BF16, ptr(logits), B, V, None, 0, C.c_int64(0), ptr(live), ptr(nxt), ptr(seq), C.c_int64(1), C.c_int64(0), None, None, i,
                                        ptr(counter)), "uvx_greedy_select")

        def dev(i):      # (the bare entry point on buffers made once, like `plain`: ops.greedy_select_penalized allocates its outputs per call)
            check(lib.uvx_greedy_select_penalized(stream_ptr(), _lib.BF16, ptr(logits), B, V, penalty, ptr(seen), seen.shape[1], None, None, 0, 0, ptr(live),
                                                  ptr(nxt), ptr(seq), 1, 0, None, None, i, ptr(counter)), "uvx_greedy_select_penalized")
        calls = {"dev": dev,
                 "host": lambda i: torch.argmax(generation.repetition_penalty_(logits.float(), ids, penalty), dim=-1),
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
        lines.append(f"{B:>3} {spread(times['dev']):>32} {spread(times['host']):>38} {spread(times['plain']):>32}  {med['host'] / med['dev']:6.2f}x"
                     f"         {med['dev'] / med['plain']:6.2f}x   ({apart(times['host'], times['dev']) if med['host'] > med['dev'] else 'the HOST side is faster: ' + apart(times['dev'], times['host'])})")


def generate_ab(lines):
    import bench
    from ultravox_amd.config import UltravoxConfig
    from ultravox_amd.frontend import WhisperFeatureExtractor
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
    variants = {"greedy (uvx_greedy_select)": (True, {}), "penalty 1.1, penalized_select on": (True, dict(repetition_penalty=1.1)),
                "penalty 1.1, penalized_select off": (False, dict(repetition_penalty=1.1))}

    def timed(n, on, kw, reps=2):
        model.penalized_select = on
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            model.generate(audio_values=fe.logmel_device(pcm), max_new_tokens=n, eos_token_id=-1, **gb, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps
    for on, kw in variants.values():
        timed(N, on, kw, 1)
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (on, kw) in variants.items():
            ms[k].append((timed(N, on, kw) - timed(1, on, kw)) / (N - 1) * 1e3)
    lines.append("")
    lines.append(f"(b) generate() at the 8B shape of bench.py --workload c4s, B = 1, {N} new tokens; ms per decoded token: median [min .. max] over {rounds} rounds, alternating")
    for k, v in ms.items():
        lines.append(f"    {k:<36} {statistics.median(v):7.3f} [{min(v):7.3f} .. {max(v):7.3f}]")
    on, off = ms["penalty 1.1, penalized_select on"], ms["penalty 1.1, penalized_select off"]
    lines.append(f"    on against off: {apart(off, on) if statistics.median(off) > statistics.median(on) else 'the HOST loop is faster: ' + apart(on, off)}")


def main():
    out = sys.argv[1]
    lines = ["# uvx_greedy_select_penalized against the host loop's repetition penalty (tools/penalized_select_ab.py; MI355X, one process, one call)"]
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
