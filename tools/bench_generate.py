#!/usr/bin/env python3
"""Measures the device-side generation path on the GPU and writes profiles/generate_bench.json:

  sampler   exl3_sample per mode at m = 1 and 16 rows of 128 256 fp16 logits against torch doing the same job on the same logits in the same process
            (argmax; softmax + multinomial; top-k / sort + cumsum for top-p).  exl3_sample as a graph of 50 calls (device time), torch as eager launches in a tight loop.
  generate  tokens/s of the replayed generation loop (decode step + sampler + token feed in one graph, no host read) against the host-stepped loop (graph of the
            decode step, logits copied to the host, numpy argmax, counters advanced from the host), bench.py's --attention configuration (4 bpw mul1, 4-bit cache)
            at the 8B and 1B shapes, 8-token prompt + 256 new tokens from an empty cache.

  processors  exl3_logit_process alone at m = 1 and 16 rows of 128 256 fp16 logits (penalties over a 1024-token window; bias + bitmask only), as a graph of 50
            calls; the replayed generation loop with processors on against the same loop without them (the two alternating), and generate() under a 256-token
            budget that stops at token ~20 (stop_token_ids) against the same call without stop ids (replays and wall time, capture included).

  prompt    time to the first new token (from the call of generate(prompt, 1) until the sampled token is on the host: allocation, the uncaptured step, the
            capture and the read included) with the prompt fed through the decode step token by token (prompt_mode "decode") against the prompt ingested through
            the prefill route in chunks (prompt_mode "prefill"), the two modes alternating, at prompt lengths 8 .. 8192 on the 8B and 1B shapes; the prompt length
            where prefill mode first wins; ingest_prompt alone (device time, tokens/s) over a chunk sweep at the longest prompt, from which the default chunk
            (SyntheticEXL3Llama.gen_prefill_chunk) is taken; and the same ingestion with dequant_cache_paged switched off (timing only: the share of
            re-expanding the past for every chunk and layer).

  speculative  generate(speculative=...) (written to profiles/spec_decode_bench.json): the replayed body (m-row fused verify step + sampler + accept / draft / feed)
            at m = 1 against the plain replayed loop (the price of leaving the persistent step) and at m = 2, 3, 4, 5, 8; tokens/s with an oracle script (every
            draft accepted: the ceiling), an all-wrong script (the floor: pure overhead) and the n-gram drafter on the model's own greedy output with its
            acceptance; the break-even acceptance per m; accept + draft as one launch against two; the share of the decode attention in the m-row step at
            1000 and 16 000 cached tokens (every row re-reads the quantized K / V).

Method: device events around whole windows that end in a synchronise, every shape warmed up, windows of at least --window seconds, the two sides of a comparison
alternating in one process, min / median / max of the repeated windows reported.  A run without a GPU fails."""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

V = 128256
CALLS = 50


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "windows": len(xs)}


def timed_window(fn, reps):
    """ms of `reps` calls of fn between two device events; ends in a synchronise."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def graph_of(fn, calls):
    import torch
    fn(); torch.cuda.synchronize()
    st = torch.cuda.Stream(); st.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(st):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            for _ in range(calls):
                fn()
    torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    return g


def alternate(sides, window_s, repeats):
    """sides: {name: (callable, units per call)} -> {name: spread of us per unit}; windows of >= window_s each, the sides alternating."""
    reps = {}
    for name, (fn, units) in sides.items():
        fn(); fn()
        t = timed_window(fn, 3) / 3
        reps[name] = max(1, math.ceil(window_s * 1e3 / max(t, 1e-3)))
    out = {name: [] for name in sides}
    for _ in range(repeats):
        for name, (fn, units) in sides.items():
            out[name].append(timed_window(fn, reps[name]) * 1e3 / (reps[name] * units))
    return {name: dict(spread(v), unit="us", calls_per_window=reps[name] * sides[name][1]) for name, v in out.items()}


def bench_sampler(dev, args):
    import torch
    from exllamav3_amd import sampling
    res = {}
    gen = torch.Generator(device=dev); gen.manual_seed(1)
    for m in (1, 16):
        logits = (torch.randn((m, V), device=dev, generator=gen) * 3.0).half()
        stepw = torch.zeros((1,), dtype=torch.int64, device=dev)
        out = torch.empty((m,), dtype=torch.int32, device=dev)
        ws = sampling.workspace(m, dev)
        S = sampling.SamplerSettings

        def t_greedy(): return torch.argmax(logits, dim=-1)
        def t_sample(): return torch.multinomial(torch.softmax(logits.float() * 1.25, dim=-1), 1)

        def t_minp():
            p = torch.softmax(logits.float(), dim=-1)
            p = torch.where(p >= 0.05 * p.amax(dim=-1, keepdim=True), p, torch.zeros_like(p))
            return torch.multinomial(torch.softmax(torch.log(p) * 1.25, dim=-1), 1)

        def t_topk_topp():
            v, i = torch.topk(logits.float(), 50, dim=-1)
            p = torch.softmax(v * 1.25, dim=-1)
            c = torch.cumsum(p, dim=-1)
            keep = c <= 0.9
            keep[:, 0] = True
            return torch.gather(i, 1, torch.multinomial(torch.where(keep, p, torch.zeros_like(p)), 1))

        def t_topp():
            v, i = torch.sort(logits.float(), dim=-1, descending=True)
            p = torch.softmax(v * 1.25, dim=-1)
            c = torch.cumsum(p, dim=-1)
            keep = c <= 0.9
            keep[:, 0] = True
            return torch.gather(i, 1, torch.multinomial(torch.where(keep, p, torch.zeros_like(p)), 1))

        cases = [("mode0_greedy", S(temperature=0.0), t_greedy), ("mode1_sample", S(temperature=0.8), t_sample), ("mode2_minp", S(temperature=0.8, min_p=0.05), t_minp),
                 ("mode3_topk50_topp0.9", S(temperature=0.8, top_k=50, top_p=0.9), t_topk_topp), ("mode3_topp0.9", S(temperature=0.8, top_p=0.9), t_topp)]
        for name, st, tfn in cases:
            ka = st.kernel_args()
            ours = graph_of(lambda: sampling.sample(logits, ka, stepw, out=out, ws=ws), CALLS)
            # torch's side as eager launches in a tight loop (its ops allocate their results; what a caller of torch gets without writing a capture of his own)
            r = alternate({"exl3_sample": (ours.replay, CALLS), "torch_eager": (tfn, 1)}, args.window, args.repeats)
            r["mode"], r["launches"] = ka.mode, (1 if ka.mode < 2 else 2)
            res[f"m{m}_{name}"] = r
            print(f"m{m}_{name}", json.dumps(r), flush=True)
    return res


def bench_generate(dev, args, shape_name):
    import numpy as np
    import torch
    from exllamav3_amd import sampling
    from exllamav3_amd.llama_path import SHAPES, SyntheticEXL3Llama
    m = SyntheticEXL3Llama(SHAPES[shape_name], K=4, cb=2, device=dev, kv_bits=4, layers=args.layers or None)
    m.with_attention = True
    prompt = torch.tensor([[128000, 9906, 11, 856, 836, 374, 1234, 77]])
    P, new = prompt.shape[1], args.new_tokens
    total = P - 1 + new
    ka = sampling.SamplerSettings(temperature=0.0).kernel_args()
    ka_s = sampling.SamplerSettings(temperature=0.8, top_k=50, top_p=0.9, seed=1).kernel_args()
    gs = m.alloc_gen_state(1, new, prompt)
    table = m.embed_table()
    m.gen_step(ka); torch.cuda.synchronize()
    persistent = m._pstep is not None and not m._pstep.error()
    graphs = {}
    for nm, k in (("greedy", ka), ("sampled", ka_s)):
        m._gen_prime()
        graphs[nm] = graph_of(lambda: m.gen_step(k), 1)
    m._gen_prime()
    g_step = graph_of(m.decode_step_auto, 1)

    def device_loop(nm):
        m._gen_prime()
        for _ in range(total):
            graphs[nm].replay()

    def host_loop():
        toks = prompt[0].tolist()
        tok = toks[0]
        for s in range(total):
            m.positions.fill_(s); m.cache_seqlens.fill_(s); m.attn_lens.fill_(s + 1)
            m.x0.copy_(table[tok].view(1, -1))
            g_step.replay()
            l = m.logits[0].cpu().numpy()
            tok = toks[s + 1] if s + 1 < P else int(np.argmax(l[:V]))

    device_loop("greedy"); torch.cuda.synchronize()
    dev_tokens = gs.tokens_out[0].cpu().tolist()
    r = alternate({"device_loop_greedy": (lambda: device_loop("greedy"), total), "host_stepped_loop_greedy": (host_loop, total),
                   "device_loop_topk50_topp0.9": (lambda: device_loop("sampled"), total)}, args.window, args.repeats)
    out = {"shape": shape_name, "layers": m.n_layers, "prompt_tokens": P, "new_tokens": new, "steps_per_generation": total, "persistent_step": bool(persistent),
           "invalid_rows": int(gs.invalid.sum()), "first_tokens": dev_tokens[P - 1:P + 7]}
    for k, v in r.items():
        out[k] = dict(v, unit="us per step", tokens_per_s=round(1e6 / v["median"], 1))
    print(shape_name, json.dumps(out), flush=True)
    del m, graphs, g_step
    torch.cuda.empty_cache()
    return out


def bench_logit_process(dev, args):
    import numpy as np
    import torch
    from exllamav3_amd import sampling
    res = {}
    gen = torch.Generator(device=dev); gen.manual_seed(2)
    rng = np.random.default_rng(2)
    bias = {int(t): float(v) for t, v in zip(rng.integers(0, V, 300), rng.standard_normal(300))}
    for m in (1, 16):
        logits = (torch.randn((m, V), device=dev, generator=gen) * 3.0).half()
        out = torch.empty_like(logits)
        past = torch.randint(0, V, (m, 2048), device=dev, generator=gen).to(torch.int32)
        stepw = torch.full((1,), 2048, dtype=torch.int64, device=dev)
        bm = torch.randint(-2 ** 31, 2 ** 31 - 1, (m, (V + 31) // 32), device=dev, generator=gen).to(torch.int32)
        pen = sampling.LogitProcessors(rep_p=1.3, rep_sustain=512, rep_decay=512, pres_p=0.2, freq_p=0.3, pf_sustain=1024, pf_decay=0)
        bb = sampling.LogitProcessors(logit_bias=bias, ban_token_ids=[1, 2, 3], bitmask=bm)
        allp = sampling.LogitProcessors(rep_p=1.3, rep_sustain=512, rep_decay=512, pres_p=0.2, freq_p=0.3, pf_sustain=1024, pf_decay=0, logit_bias=bias, bitmask=bm)
        sides = {}
        for nm, pr in (("penalties_window1024", pen), ("bias_bitmask", bb), ("all", allp)):
            g = graph_of(lambda pr=pr: sampling.process_logits(logits, pr, None, past, step=stepw, out=out), CALLS)
            sides[nm] = (g.replay, CALLS)
        r = alternate(sides, args.window, args.repeats)
        for nm, v in r.items():
            res[f"m{m}_{nm}"] = v
            print(f"logit_process m{m}_{nm}", json.dumps(v), flush=True)
    return res


def bench_generate_processors(dev, args, shape_name):
    import torch
    from exllamav3_amd import sampling
    from exllamav3_amd.llama_path import SHAPES, SyntheticEXL3Llama
    m = SyntheticEXL3Llama(SHAPES[shape_name], K=4, cb=2, device=dev, kv_bits=4, layers=args.layers or None)
    m.with_attention = True
    prompt = torch.tensor([[128000, 9906, 11, 856, 836, 374, 1234, 77]])
    P, new = prompt.shape[1], args.new_tokens
    total = P - 1 + new
    ka = sampling.SamplerSettings(temperature=0.0).kernel_args()
    procs = sampling.LogitProcessors(rep_p=1.3, rep_sustain=512, rep_decay=512, pres_p=0.2, freq_p=0.3, pf_sustain=1024, pf_decay=0, logit_bias={12345: 2.0},
                                     ban_token_ids=[128001, 128009])
    gs = m.alloc_gen_state(1, new, prompt)
    gs.proc_logits = torch.empty_like(m.logits)
    m.gen_step(ka, procs); torch.cuda.synchronize()
    graphs = {}
    for nm, pr in (("off", None), ("on", procs)):
        m._gen_prime()
        graphs[nm] = graph_of(lambda pr=pr: m.gen_step(ka, pr), 1)

    def device_loop(nm):
        m._gen_prime()
        for _ in range(total):
            graphs[nm].replay()

    r = alternate({"device_loop_greedy": (lambda: device_loop("off"), total), "device_loop_greedy_processors": (lambda: device_loop("on"), total)},
                  args.window, args.repeats)
    out = {"shape": shape_name, "layers": m.n_layers, "steps_per_generation": total, "invalid_rows": int(gs.invalid.sum())}
    for k, v in r.items():
        out[k] = dict(v, unit="us per step", tokens_per_s=round(1e6 / v["median"], 1))
    out["processors_cost_us_per_step"] = round(out["device_loop_greedy_processors"]["median"] - out["device_loop_greedy"]["median"], 3)
    del graphs
    # the stop path: generate() under a 256-token budget, stopped at token ~20 (wall time of the whole call: allocation, the uncaptured step, the capture, the replays)
    m.with_attention = False
    plain = m.generate(prompt[0], new)
    stop = int(plain[20])
    first = plain.tolist().index(stop)
    stop_res = {"stop_token_index": first}
    for nm, kw in (("without_stop_ids", {}), ("with_stop_ids", {"stop_token_ids": [stop]})):
        walls = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = m.generate(prompt[0], new, **kw)
            walls.append((time.perf_counter() - t0) * 1e3)
        stop_res[nm] = {"wall_ms": spread(walls), "graph_replays": m.gen_stats["graph_replays"], "host_reads": m.gen_stats["host_reads"], "tokens_returned": int(got.numel())}
    out["stop_path"] = stop_res
    print("processors", shape_name, json.dumps(out), flush=True)
    del m
    torch.cuda.empty_cache()
    return out


def bench_prompt(dev, args, shape_name):
    import torch
    from exllamav3_amd import ext
    from exllamav3_amd.llama_path import SHAPES, SyntheticEXL3Llama
    lengths = [int(x) for x in args.prompt_lengths.split(",")]
    chunks = [int(x) for x in args.prompt_chunks.split(",")]
    m = SyntheticEXL3Llama(SHAPES[shape_name], K=4, cb=2, device=dev, kv_bits=4, layers=args.layers or None, max_ctx=(max(lengths) + 1 + 255) // 256 * 256)
    gen = torch.Generator(); gen.manual_seed(3)
    out = {"shape": shape_name, "layers": m.n_layers, "default_chunk": m.gen_prefill_chunk, "ttft_ms": {},
           "method": "wall time of whole generate(prompt, 1) calls (ttft_ms), device time of ingest_prompt (ingest_chunk_sweep); one warm call, then %d windows of >= %.1f s per side, "
                     "sides alternating" % (args.repeats, args.window)}

    def windows(sides):
        """sides: {name: callable} -> {name: spread of ms per call}: one warm call each (it sizes the window), then windows of >= args.window s, alternating."""
        reps = {}
        for name, fn in sides.items():
            reps[name] = max(1, math.ceil(args.window * 1e3 / max(timed_window(fn, 1), 1e-3)))
        res = {name: [] for name in sides}
        for _ in range(args.repeats):
            for name, fn in sides.items():
                res[name].append(timed_window(fn, reps[name]) / reps[name])
        return {name: dict(spread(v), unit="ms", calls_per_window=reps[name]) for name, v in res.items()}

    m.generate(torch.randint(0, V, (8,), generator=gen), 1)                            # plans, the persistent step's first run
    first_win = None
    for P in lengths:
        prompt = torch.randint(0, V, (P,), generator=gen)
        r = windows({"decode": lambda: m.generate(prompt, 1), "prefill": lambda: m.generate(prompt, 1, prompt_mode="prefill")})
        r["prefill_chunks"] = m.gen_stats.get("prefill_chunks")
        r["speedup"] = round(r["decode"]["median"] / r["prefill"]["median"], 2)
        for k in ("decode", "prefill"):
            r[k]["prompt_tokens_per_s"] = round((P - 1) / (r[k]["median"] * 1e-3), 1)
        if first_win is None and r["prefill"]["median"] < r["decode"]["median"]:
            first_win = P
        out["ttft_ms"][str(P)] = r
        print("prompt", shape_name, P, json.dumps(r), flush=True)
    out["prefill_first_wins_at"] = first_win
    # ingestion alone over the chunk sweep at the longest prompt
    P = max(lengths)
    m.alloc_gen_state(1, 1, torch.randint(0, V, (1, P), generator=gen))
    sweep = windows({str(c): (lambda c=c: m.ingest_prompt(P - 1, c)) for c in chunks})
    for c, v in sweep.items():
        v["tokens_per_s"] = round((P - 1) / (v["median"] * 1e-3), 1)
    out["ingest_chunk_sweep"] = dict(sweep, prompt_tokens=P - 1)
    best = min(sweep, key=lambda c: sweep[c]["median"])
    out["best_chunk"] = int(best)
    real = ext.dequant_cache_paged
    try:
        ext.dequant_cache_paged = lambda *a, **k: None                                # timing only: the attention then reads stale pages
        off = windows({"no_dequant": lambda: m.ingest_prompt(P - 1, int(best))})["no_dequant"]
    finally:
        ext.dequant_cache_paged = real
    out["dequant_cache_paged_share"] = round(1.0 - off["median"] / sweep[best]["median"], 4)
    out["ingest_without_dequant_ms"] = off
    print("prompt", shape_name, json.dumps({k: out[k] for k in ("prefill_first_wins_at", "ingest_chunk_sweep", "best_chunk", "dequant_cache_paged_share")}), flush=True)
    del m
    torch.cuda.empty_cache()
    return out


def bench_speculative(dev, args, shape_name):
    import copy
    import torch
    from exllamav3_amd import sampling
    from exllamav3_amd.llama_path import SHAPES, SyntheticEXL3Llama
    m = SyntheticEXL3Llama(SHAPES[shape_name], K=4, cb=2, device=dev, kv_bits=4, layers=args.layers or None)
    ctx = m.max_ctx
    m.with_attention = True
    prompt = torch.tensor([128000, 9906, 11, 856, 836, 374, 1234, 77])
    P, new = prompt.numel(), args.new_tokens
    ka = sampling.SamplerSettings(temperature=0.0).kernel_args()
    out = {"shape": shape_name, "layers": m.n_layers, "prompt_tokens": P, "new_tokens": new, "max_ctx": ctx}
    # the plain loop: prompt ingested, then `new` replays of gen_step (persistent step where it applies)
    gs = m.alloc_gen_state(1, new, prompt.view(1, -1))
    m.gen_step(ka); torch.cuda.synchronize()
    out["persistent_step"] = bool(m._pstep is not None and not m._pstep.error())
    m._gen_prime_prefilled()
    g_plain = graph_of(lambda: m.gen_step(ka), 1)

    def plain_loop():
        # _gen_prime_prefilled without the ingestion (the prompt's K / V stay where the first call put them, as they do on the speculative side)
        m._gen_prime()
        m.positions.fill_(P - 2); m.cache_seqlens.fill_(P - 2); m.attn_lens.fill_(P - 1)
        gs.step.fill_(P - 2)
        gs.tokens_out[:, :P - 2] = gs.forced[:, 1:P - 1]
        sampling.gen_feed(None, gs.forced, gs.embed, m.x0, gs.tokens_out, m.positions, m.cache_seqlens, m.attn_lens, gs.invalid, gs.step, vocab=m.shape.vocab)
        for _ in range(new):
            g_plain.replay()

    sides = {"plain_generate": (plain_loop, new)}
    info = {}
    for rows in (1, 2, 3, 4, 5, 8):
        k = rows - 1
        mm = copy.copy(m)                                                 # the weights shared, a state of its own
        mm.spec_fold = True
        script = torch.full((ctx,), -1, dtype=torch.int32, device=dev)
        sp = mm.alloc_spec_state(k, new, prompt, sampling.SpeculativeSettings(script=script.cpu()))
        mm._spec_ingest(); mm._spec_prime()
        mm.spec_step(ka); torch.cuda.synchronize()
        mm._spec_prime()
        g_script = graph_of(lambda mm=mm: mm.spec_step(ka), 1)
        mm._spec_prime()

        def loop(mm=mm, g=g_script, n=new):
            mm._spec_prime()
            for _ in range(n):
                g.replay()

        loop(); torch.cuda.synchronize()                                  # no drafts: one token per round = this m's own greedy continuation
        truth = mm.spec.tokens_out[:new].clone()
        assert int(mm.spec.state[sampling.SPEC_PRODUCED]) == new and not int(mm.spec.state[sampling.SPEC_INVALID])
        oracle, wrong = script.clone(), script.clone()
        oracle[P:P + new] = truth
        wrong[P:P + new] = (truth + 1) % m.shape.vocab

        def scripted(table, n, mm=mm, g=g_script):
            mm.spec.script.copy_(table)
            mm._spec_prime()
            for _ in range(n):
                g.replay()

        r_oracle = math.ceil(new / rows)
        scripted(oracle, r_oracle); torch.cuda.synchronize()
        assert int(mm.spec.state[sampling.SPEC_PRODUCED]) == new and torch.equal(mm.spec.tokens_out[:new], truth), "the oracle script changed the tokens"
        sides[f"m{rows}_body_all_wrong_script"] = (lambda wrong=wrong, scripted=scripted: scripted(wrong, new), new)
        info[rows] = {"rounds_oracle": r_oracle}
        if k >= 1:
            sides[f"m{rows}_oracle_script"] = (lambda oracle=oracle, scripted=scripted, r=r_oracle: scripted(oracle, r), new)
            ng = copy.copy(m)
            ng.spec_fold = True
            ng.alloc_spec_state(k, new, prompt, sampling.SpeculativeSettings(num_draft_tokens=k))
            ng._spec_ingest(); ng._spec_prime()
            ng.spec_step(ka); torch.cuda.synchronize()
            ng._spec_prime()
            g_ng = graph_of(lambda ng=ng: ng.spec_step(ka), 1)
            ng._spec_prime()
            rounds = 0
            while int(ng.spec.live.cpu()):
                g_ng.replay(); rounds += 1
            st = ng.spec.state.tolist()
            assert st[sampling.SPEC_PRODUCED] == new and torch.equal(ng.spec.tokens_out[:new], truth), "the n-gram drafter changed the tokens"
            info[rows].update(rounds_ngram=rounds, ngram_drafted=st[sampling.SPEC_DRAFTED], ngram_accepted=st[sampling.SPEC_ACCEPTED],
                              ngram_acceptance=round(st[sampling.SPEC_ACCEPTED] / max(st[sampling.SPEC_DRAFTED], 1), 4),
                              ngram_tokens_per_round=round(new / rounds, 3))

            def ng_loop(ng=ng, g=g_ng, n=rounds):
                ng._spec_prime()
                for _ in range(n):
                    g.replay()

            sides[f"m{rows}_ngram"] = (ng_loop, new)
        if rows == 4:
            tw = copy.copy(m)
            tw.spec_fold = False
            tw.alloc_spec_state(k, new, prompt, sampling.SpeculativeSettings(script=wrong.cpu()))
            tw._spec_ingest(); tw._spec_prime()
            tw.spec_step(ka); torch.cuda.synchronize()
            tw._spec_prime()
            g_tw = graph_of(lambda tw=tw: tw.spec_step(ka), 1)

            def tw_loop(tw=tw, g=g_tw):
                tw._spec_prime()
                for _ in range(new):
                    g.replay()

            sides["m4_body_all_wrong_script_two_launches"] = (tw_loop, new)
    r = alternate(sides, args.window, args.repeats)
    plain = r["plain_generate"]["median"]
    out["plain_generate"] = dict(r["plain_generate"], unit="us per token", tokens_per_s=round(1e6 / plain, 1))
    for rows, inf in info.items():
        body = r[f"m{rows}_body_all_wrong_script"]
        e = dict(inf, body_us_per_replay=body, floor_tokens_per_s=round(1e6 / body["median"], 1), body_over_plain=round(body["median"] / plain, 4))
        if rows > 1:
            # the round costs body / plain plain-steps and yields 1 + a (rows - 1) tokens at per-draft acceptance a (drafts always full): break-even a
            e["break_even_tokens_per_round"] = round(body["median"] / plain, 4)
            e["break_even_acceptance_per_draft"] = round((body["median"] / plain - 1.0) / (rows - 1), 4)
            o, n = r[f"m{rows}_oracle_script"], r[f"m{rows}_ngram"]
            e["ceiling_oracle_script"] = dict(o, unit="us per token", tokens_per_s=round(1e6 / o["median"], 1))
            e["ngram"] = dict(n, unit="us per token", tokens_per_s=round(1e6 / n["median"], 1))
        out[f"m{rows}"] = e
    out["m4_two_launches_body_us_per_replay"] = r["m4_body_all_wrong_script_two_launches"]
    print("speculative", shape_name, json.dumps(out), flush=True)
    # the decode attention's share of the m-row fused step at long contexts: rows of ONE sequence, each re-reading the quantized K / V up to its own length
    att = {}
    for pos in (1000, 16000):
        s2 = {}
        for rows in (1, 4, 8):
            for on in (True, False):
                mm = copy.copy(m)
                mm.with_attention = on
                mm.max_ctx = 16384 + 512                                   # (only allocation reads it)
                mm._alloc_state(rows, pos, None, one_sequence=True)
                ar = torch.arange(rows, dtype=torch.int32, device=dev)
                mm.positions.copy_(pos + ar); mm.cache_seqlens.copy_(pos + ar); mm.attn_lens.copy_(pos + 1 + ar)
                mm.attn_pos = pos + rows
                mm.attn_ws = torch.empty((rows * mm.hq * ((pos + rows + 32) // 32) * 132,), dtype=torch.float, device=dev)
                g = graph_of(mm.decode_step_fused, 1)
                s2[f"m{rows}_{'attention' if on else 'no_attention'}"] = (lambda g=g, keep=mm: g.replay(), 1)
        r2 = alternate(s2, args.window / 2, args.repeats)
        e = {}
        for rows in (1, 4, 8):
            a, b = r2[f"m{rows}_attention"]["median"], r2[f"m{rows}_no_attention"]["median"]
            e[f"m{rows}"] = {"step_us": a, "step_without_attention_us": b, "attention_share": round(1.0 - b / a, 4)}
        att[str(pos)] = e
        print("speculative attention share", shape_name, pos, json.dumps(e), flush=True)
    out["attention_share_of_fused_step"] = att
    del m, sides
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.0, help="seconds per timed window (at least)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--new-tokens", type=int, default=256)
    ap.add_argument("--layers", type=int, default=0, help="debug: fewer layers (invalidates the number)")
    ap.add_argument("--skip", default="", help="comma list of: sampler, 8b, 1b, processors, prompt, speculative (a skipped section keeps what --out already holds)")
    ap.add_argument("--spec-out", default=os.path.join(ROOT, "profiles", "spec_decode_bench.json"), help="section speculative: its own result file")
    ap.add_argument("--prompt-lengths", default="8,64,512,2048,8192", help="section prompt: prompt lengths")
    ap.add_argument("--prompt-chunks", default="512,1024,2048,4096", help="section prompt: the chunk sweep of ingest_prompt")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generate_bench.json"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_generate.py: needs a GPU")
    from exllamav3_amd import ext
    dev = torch.device("cuda:0")
    ext.init(0)
    ext.set_gemv_variant(1)
    skip = set(args.skip.split(","))
    res = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    res.update({"device": torch.cuda.get_device_name(0), "method": "device events around windows ending in a synchronise; >= %.1f s per window; sides alternating; %d windows per side"
           % (args.window, args.repeats), "when": time.strftime("%Y-%m-%d")})
    if "sampler" not in skip:
        res["sampler_us_per_call"] = bench_sampler(dev, args)
    res.setdefault("generate", {})
    for nm, shape in (("8b", "llama-3.1-8b"), ("1b", "llama-3.2-1b")):
        if nm not in skip:
            res["generate"][shape] = bench_generate(dev, args, shape)
    if "processors" not in skip:
        res["logit_process_us_per_call"] = bench_logit_process(dev, args)
        res["generate_processors"] = {shape: bench_generate_processors(dev, args, shape) for shape in ("llama-3.1-8b", "llama-3.2-1b")}
    if "prompt" not in skip:
        res["prompt"] = {shape: bench_prompt(dev, args, shape) for shape in ("llama-3.1-8b", "llama-3.2-1b")}
    if "speculative" not in skip:
        spec = {"device": res["device"], "method": res["method"], "when": res["when"],
                "speculative": {shape: bench_speculative(dev, args, shape) for shape in ("llama-3.1-8b", "llama-3.2-1b")}}
        os.makedirs(os.path.dirname(args.spec_out), exist_ok=True)
        with open(args.spec_out, "w") as f:
            json.dump(spec, f, indent=1)
        print("wrote", args.spec_out)
    if not {"sampler", "8b", "1b", "processors", "prompt"} <= skip:
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", args.out)


if __name__ == "__main__":
    main()
