"""A/B of the token-ban score processors on the device (uvx_greedy_select_banned / uvx_sample_select_banned) against the host policy they replace, on
the GPU; writes the table of profiles/banned_select_ab.txt.

  python tools/banned_select_ab.py OUT.txt [--skip-generate]

Rules everywhere: no_repeat_ngram_size 3, 90 suppressed ids, four bad words (one of one token, three of two / three tokens), repetition penalty 1.1.
(a) one call on the same bf16 logits [B, 128256] over a 512-token row: uvx_greedy_select_banned (rule prologue + penalty + argmax + bookkeeping, one
    launch) against what the generic loop runs for the same decision - logits.float(), generation.ScoreProcessors.__call__ (gather / where / scatter_
    for the penalty, unfold / nonzero / index for the n-gram rule, the bad-word and suppress masks) and argmax; the loop's cat / where / isin / any
    bookkeeping is NOT in that number - and, next to them, uvx_greedy_select_penalized on the same logits (what the bans add to the penalty).
    Device events around blocks of 50 calls, the versions alternating, 5 rounds each = 250 timed calls; median [min .. max] of the rounds' per-call
    means.
(b) the same under sampling (temperature 0.7, top_k 50, top_p 0.9): uvx_sample_select_banned against logits.float() + ScoreProcessors.__call__ +
    UltravoxModel._sample.
(c) ms per decoded token of generate(max_new_tokens=64, eos_token_id=-1) under these rules at the 8B inference shape of `bench.py --workload c4s`
    (its config, imported), B = 1: model.banned_select on against off (UVX_GREEDY_SELECT=0 gives the same host loop).  As bench.py does it:
    (whole call - a max_new_tokens=1 call) / 63, host clock around a device synchronise, the versions alternating over 4 rounds.
"""
import ctypes as C
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V, N_ROW, PENALTY = 128256, 512, 1.1


def rule_kwargs(gen_device="cpu"):
    g = torch.Generator(device=gen_device).manual_seed(1)
    ids = torch.randint(0, V, (90 + 9,), generator=g, device=gen_device).tolist()
    return dict(no_repeat_ngram_size=3, suppress_tokens=ids[:90], bad_words_ids=[[ids[90]], ids[91:93], ids[93:96], ids[96:99]])


def spread(v):
    return f"{statistics.median(v):9.1f} [{min(v):8.1f} .. {max(v):8.1f}]"


def apart(slow, fast):
    return "min of the slower side's rounds above the max of the faster side's" if min(slow) > max(fast) else "the rounds OVERLAP"


def verdict(host, dev):
    return apart(host, dev) if statistics.median(host) > statistics.median(dev) else "the HOST side is faster: " + apart(dev, host)


def kernel_ab(lines, sampling):
    from ultravox_amd import _lib, generation, ops
    from ultravox_amd._lib import check, ptr, stream_ptr
    from ultravox_amd.model import UltravoxModel
    block, rounds = 50, 5
    warp = dict(temperature=0.7, top_k=50, top_p=0.9)
    what = "uvx_sample_select_banned" if sampling else "uvx_greedy_select_banned"
    host_name = "float + ScoreProcessors + " + ("_sample" if sampling else "argmax")
    sibling = "uvx_sample_select_penalized" if sampling else "uvx_greedy_select_penalized"
    lines.append(f"({'b' if sampling else 'a'}) one call, bf16 logits [B, {V}] = 3 * randn (seed 0), a row of {N_ROW} ids, rules as above"
                 + (f", {warp}" if sampling else "") + f"; us per call: median [min .. max] over {rounds} rounds of {block} calls, alternating")
    lines.append(f"{'B':>3} {what:>32} {host_name:>38} {sibling:>32}  host / device   device / penalty only")
    gen = torch.Generator(device="cuda").manual_seed(0)
    kw = rule_kwargs()
    for B in (1, 8):
        logits = (3.0 * torch.randn(B, V, device="cuda", generator=gen)).bfloat16()
        ids = torch.randint(0, V, (B, N_ROW), device="cuda", generator=gen)
        procs = generation.ScoreProcessors(kw, N_ROW, 64, [-1], PENALTY)
        assert procs.on_device(V)
        lists = procs.device_rules("cuda")
        rules = _lib.BanRules(**{f: ptr(v) if isinstance(v, torch.Tensor) else v for f, v in lists.items()})
        flags = procs.step_flags(N_ROW)
        seen, seen2 = ops.seen_mark(ids, V), ops.seen_mark(ids, V)
        words = seen.shape[1]
        ban = torch.empty(B, words, device="cuda", dtype=torch.int32)
        live = torch.ones(B, device="cuda", dtype=torch.int32)
        seq = torch.zeros(B, N_ROW + 1, device="cuda", dtype=torch.int64)
        seq[:, :N_ROW] = ids
        nxt = torch.empty(B, device="cuda", dtype=torch.int64)
        counter = torch.zeros(2, device="cuda", dtype=torch.int32)
        lib = _lib.lib()
        book = lambda i: (None, 0, 0, ptr(live), ptr(nxt), ptr(seq), N_ROW + 1, N_ROW, None, None, i, ptr(counter))
        w = (warp["temperature"], warp["top_k"], warp["top_p"], 0.0, 1, 0)

        # (the bare entry points on buffers made once: the ops wrappers allocate their outputs per call)
        def dev(i):
            if sampling:
                check(lib.uvx_sample_select_banned(stream_ptr(), _lib.BF16, ptr(logits), B, V, PENALTY, ptr(seen), words, *w, i, None, None, C.byref(rules), flags,
                                                   ptr(ban), words, *book(i)), what)
            else:
                check(lib.uvx_greedy_select_banned(stream_ptr(), _lib.BF16, ptr(logits), B, V, PENALTY, ptr(seen), words, None, C.byref(rules), flags, ptr(ban),
                                                   words, *book(i)), what)

        def pen(i):
            if sampling:
                check(lib.uvx_sample_select_penalized(stream_ptr(), _lib.BF16, ptr(logits), B, V, PENALTY, ptr(seen2), words, *w, i, None, None, *book(i)), sibling)
            else:
                check(lib.uvx_greedy_select_penalized(stream_ptr(), _lib.BF16, ptr(logits), B, V, PENALTY, ptr(seen2), words, None, *book(i)), sibling)

        def host(i):
            scores = procs(ids, logits.float())
            return UltravoxModel._sample(scores, warp["temperature"], warp["top_k"], warp["top_p"], None) if sampling else torch.argmax(scores, dim=-1)
        calls = {"dev": dev, "host": host, "pen": pen}
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
        lines.append(f"{B:>3} {spread(times['dev']):>32} {spread(times['host']):>38} {spread(times['pen']):>32}  {med['host'] / med['dev']:6.2f}x"
                     f"         {med['dev'] / med['pen']:6.2f}x   ({verdict(times['host'], times['dev'])})")
    lines.append("")


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
    rules = dict(rule_kwargs(), repetition_penalty=PENALTY)
    variants = {"greedy (uvx_greedy_select)": (True, {}), "penalty 1.1 alone (uvx_greedy_select_penalized)": (True, dict(repetition_penalty=PENALTY)),
                "rules + penalty, banned_select on": (True, rules), "rules + penalty, banned_select off": (False, rules)}

    def timed(n, on, kw, reps=2):
        model.banned_select = on
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            model.generate(audio_values=fe.logmel_device(pcm), max_new_tokens=n, eos_token_id=-1, **gb, **kw)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps
    tokens = {}
    for on in (True, False):
        model.banned_select = on
        tokens[on] = model.generate(audio_values=fe.logmel_device(pcm), max_new_tokens=N, eos_token_id=-1, **gb, **rules)
    same = torch.equal(tokens[True], tokens[False])
    for on, kw in variants.values():
        timed(N, on, kw, 1)
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, (on, kw) in variants.items():
            ms[k].append((timed(N, on, kw) - timed(1, on, kw)) / (N - 1) * 1e3)
    model.banned_select = True
    lines.append(f"(c) generate() at the 8B shape of bench.py --workload c4s, B = 1, {N} new tokens; ms per decoded token: median [min .. max] over {rounds} rounds, alternating")
    for k, v in ms.items():
        lines.append(f"    {k:<48} {statistics.median(v):7.3f} [{min(v):7.3f} .. {max(v):7.3f}]")
    lines.append(f"    on against off: {verdict(ms['rules + penalty, banned_select off'], ms['rules + penalty, banned_select on'])}; the two loops' tokens are "
                 f"{'equal' if same else 'NOT equal (bf16 logits: torch may round the penalty another way)'}")


def main():
    out = sys.argv[1]
    lines = ["# the banned selectors against the host loop's score processors (tools/banned_select_ab.py; MI355X, one process, one call)",
             "# rules: no_repeat_ngram_size 3, 90 suppressed ids, four bad words, repetition penalty 1.1", ""]
    kernel_ab(lines, sampling=False)
    kernel_ab(lines, sampling=True)
    if "--skip-generate" not in sys.argv:
        generate_ab(lines)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
