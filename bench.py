#!/usr/bin/env python
"""
bench.py — TikZ tokens/sec + MCTS rollouts/sec of the MI355X-native DeTikZify hot path.

Metric (BASELINE.json): TikZ tokens/sec + MCTS rollouts/sec, detikzify-ds-7b, 1 image, N MI355X.
One "step" = one rollout of the hot path through the product API (model.generate, the call
DetikzifyGenerator.generate makes, reference infer/generate.py:218-227): image already preprocessed
on the host -> ViT (666 GF) -> projector -> 243-token prefill -> 512 decoded tokens (EOS suppressed:
fixed work) with bad_words/begin-suppress processors, one D2H per token.  `value` is
generated tokens / wall time of the whole step loop (ViT + prefill INCLUDED); the decode-only rate and
the prefill time are reported beside it.  N > 1 (torchrun, one rank per GPU): every rank runs its own
independent rollouts on a full replica (root-parallel rollouts), the generated TikZ strings
are gathered to rank 0 over RCCL inside the timed region; scaling is weak.

A plain run sets up, warms up, times --steps rollouts and prints the headline line (`value`, `ms_per_step`, the decode-only
rate, prefill / ViT times).  `--dump-outputs DIR` writes what the last timed rollout returned (DIR/sequences.npy: the token ids
of model.generate, as float64).  Everything below runs only with `--full`.

Phases after the headline loop, with --full (each can be switched off):
  batched_rollouts  B independent sampled rollouts per GPU as ONE batched decode (the weights stream once per step)
  mcts              the search itself (DetikzifyGenerator / MonteCarlo, reference semantics): `sequential` = ONE tree per
                    GPU, expansion k+1 selects on what expansion k back-propagated (reference infer/generate.py:195-207,
                    305-353; with N ranks this is root parallelisation over the ranks, seeds 1000 + rank); `parallel` =
                    `--mcts-trees` independent trees per GPU decoded as one batch.  Reward: SelfSim on the device ViT of
                    the SYNTHETIC renderer's image (no TeX on the box: a stub-reward number, never to be mixed with
                    real-LaTeX numbers).  Each with its fraction of the decode-step HBM roofline.
  roofline          dominant kernel (RMSNorm + gate/up GEMV + SiLU*mul, 44 % of the weight bytes): duration measured
                    live with HIP events on the library's stream in a probe pass of plain launches; HBM peak 8 TB/s
  cpu_baseline      the reference's arithmetic engine — the installed HuggingFace LlamaForCausalLM with its KV cache, bf16,
                    on the SAME weights (copied back from the device), image prefix from the oracle's glue — timed on the host
                    cores; its greedy tokens are compared with the device's (`parity_tokens_identical`); the oracle port and
                    BASELINE config 1 (ds-1.3b shape on the CPU) ride along as further entries
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (guides/MI355X_MICROARCH.md); ~6.3 TB/s achievable
DOMINANT_KERNEL_SOURCE = ROOT / "detikzify_amd" / "csrc" / "kernels_decode.hip"


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--model", default="detikzify-ds-7b")
    ap.add_argument("--new-tokens", type=int, default=512)
    ap.add_argument("--full", action="store_true", help="after the headline: secondary rooflines, batched rollouts, MCTS, the dominant "
                    "kernel's roofline and the CPU baselines (a plain run prints the headline only)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write the last timed rollout's output (sequences.npy: "
                    "prompt + generated token ids, float64) to DIR")
    ap.add_argument("--sample", action="store_true", help="sampling decode (T=.8, p=.95) instead of greedy")
    ap.add_argument("--reuse", action="store_true", help="SURVEY §8 f1: reuse image embeds / prefix KV across rollouts")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-tokens", type=int, default=16, help="greedy tokens of the CPU baseline (BASELINE.md §3: 16 for the 7B models)")
    ap.add_argument("--cpu-budget", type=float, default=30.0, help="seconds of CPU decode per baseline entry before it stops early")
    ap.add_argument("--no-cpu-config1", action="store_true", help="skip the BASELINE config 1 entry (ds-1.3b shape on the host CPU)")
    ap.add_argument("--probe-tokens", type=int, default=64)
    ap.add_argument("--probe-chain-reps", type=int, default=8, help="passes over all layers of the dominant kernel timed between one HIP event pair")
    ap.add_argument("--weight-format", default="bf16", choices=["bf16", "fp8"],
                    help="fp8 = e4m3 decoder weights with per-row 2^e scales (BASELINE config 5, cl-7b)")
    ap.add_argument("--skip-batched", action="store_true", help="allocate the --batch slots (for the MCTS phase) but skip the "
                    "batched_rollouts phase itself")
    ap.add_argument("--batch-images", type=int, default=1, help="spread the rollouts of the batched phase over this many "
                    "different images (BASELINE config 5: 8 images x 4 rollouts = --batch 32 --batch-images 8)")
    ap.add_argument("--batch", type=int, default=64, help="independent rollouts decoded as one batch per GPU in the "
                    "'batched_rollouts' phase and slots available to the MCTS trees (0 = neither); the headline value stays batch 1")
    ap.add_argument("--mcts-trees", type=int, default=-1, help="trees per GPU of the parallel MCTS phase (-1 = as many as --batch, 0 = skip)")
    ap.add_argument("--mcts-expansions", type=int, default=2, help="rollouts per tree in the parallel MCTS phase")
    ap.add_argument("--mcts-seq-expansions", type=int, default=3, help="rollouts of the sequential (one tree per GPU) search, 0 = skip")
    ap.add_argument("--mcts-oversubscribe", type=float, default=1.5, help="mcts.parallel_oversubscribed: this many times --mcts-trees trees "
                    "taking turns in the --mcts-trees decode slots (<= 1: skip)")
    ap.add_argument("--no-config4", action="store_true", help="skip mcts.config4 (BASELINE configs[3]: 16 rollouts of one image over the ranks)")
    ap.add_argument("--no-config5", action="store_true", help="skip mcts.config5 (BASELINE configs[4]: cl-7b fp8, 8 images x 32 rollouts over the ranks)")
    ap.add_argument("--no-rank-shapes", action="store_true", help="skip mcts.config4.rank_shape / mcts.config5.rank_shape: what ONE rank of an "
                                                                   "N = 2 / 4 / 8 job decodes (16/N trees; 8/N images), run on this GPU at N = 1, and "
                                                                   "the whole-job rate that predicts (the path has no data-path collective)")
    ap.add_argument("--config5-model", default="detikzify-cl-7b")
    ap.add_argument("--config5-images", type=int, default=8)
    ap.add_argument("--config5-trees", type=int, default=8, help="trees per image (x --config5-expansions = 32 rollouts per image)")
    ap.add_argument("--config5-expansions", type=int, default=4)
    ap.add_argument("--reward-latency", type=float, nargs="*", default=[], help="f3 measurement: emulate a LaTeX run of S seconds per reward "
                    "(S values, e.g. 1 5) with and without the compile pool, 1 tree and --mcts-trees trees")
    return ap.parse_args()


def ragged_pipeline_class(base, n_new, lo_frac=0.25):
    """A pipeline whose rollouts stop after a pseudo-random number of new tokens in [lo_frac * n_new, n_new] (a function of the
    rollout's sampling seed): real rollouts end at EOS at different lengths, synthetic weights practically never sample EOS,
    and equal-length rollouts are the easiest schedule a batch engine can get (every tree hits its reward on the same step)."""
    lo = max(1, int(n_new * lo_frac))

    class RaggedPipeline(base):
        def _generator(self, *a, **kw):
            g = super()._generator(*a, **kw)
            inner, budget = g.generate, {**self.gen_kwargs, **kw}.get("max_length")

            def generate(input_ids, seed=0, **k):
                h = (int(seed) * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03) & ((1 << 64) - 1)
                h ^= h >> 31
                length = lo + h % (n_new - lo + 1)
                return inner(input_ids, seed=seed, max_length=min(budget, int(input_ids.numel()) + length), **k)
            g.generate = generate
            return g
    return RaggedPipeline


# ------------------------------------------------------------------------------------------------ CPU baselines
def _hf_llama(cfg, weights):
    """installed transformers LlamaForCausalLM (the class the reference's DetikzifyForCausalLM subclasses,
    v1/modeling_detikzify.py:203) over the given bf16 tensors — no random init, no copies"""
    import torch
    from transformers import LlamaConfig, LlamaForCausalLM
    from transformers.models.llama.modeling_llama import LlamaRotaryEmbedding
    if cfg.get("rope_type") == "llama3":
        rope = {"rope_type": "llama3", "factor": cfg["rope_factor"], "low_freq_factor": cfg["rope_low_freq_factor"],
                "high_freq_factor": cfg["rope_high_freq_factor"],
                "original_max_position_embeddings": cfg["rope_original_max_position"]}
    else:
        rope = {"rope_type": "linear", "factor": cfg["rope_factor"] or 1.0}
    hc = LlamaConfig(hidden_size=cfg["hidden"], intermediate_size=cfg["ffn"], num_hidden_layers=cfg["layers"],
                     num_attention_heads=cfg["heads"], num_key_value_heads=cfg.get("kv_heads") or cfg["heads"],
                     head_dim=cfg["head_dim"], vocab_size=cfg["vocab"], rms_norm_eps=cfg["rms_eps"],
                     max_position_embeddings=cfg["max_positions"], rope_theta=cfg["rope_theta"], rope_scaling=rope,
                     attention_bias=False, tie_word_embeddings=False, bos_token_id=1, eos_token_id=2, pad_token_id=0)
    with torch.device("meta"):
        hf = LlamaForCausalLM(hc)
    sd = {k: weights[k].to(torch.bfloat16) for k in hf.state_dict()}
    hf.load_state_dict(sd, strict=True, assign=True)
    hf.model.rotary_emb = LlamaRotaryEmbedding(hc)          # its buffers are not in the state dict: rebuild them off meta
    return hf.eval()


def _interleave_memory() -> bool:
    """MPOL_INTERLEAVE over all NUMA nodes for what THIS thread allocates from now on (set_mempolicy(2), no libnuma needed): the
    baseline's 13 GB of weights then sit on both sockets instead of the one the first-touching thread ran on (round 5: a probe that
    read 46 GB/s on a 2-socket EPYC — VERDICT r5 weak 4).  False = not permitted / single node: the run goes on with local policy."""
    try:
        import ctypes
        nodes = [int(p.name[4:]) for p in Path("/sys/devices/system/node").glob("node[0-9]*")]
        if len(nodes) < 2:
            return False
        mask = ctypes.c_ulong(sum(1 << n for n in nodes if n < 64))
        libc = ctypes.CDLL(None, use_errno=True)
        return libc.syscall(238, 3, ctypes.byref(mask), ctypes.c_ulong(65)) == 0        # SYS_set_mempolicy (x86-64), MPOL_INTERLEAVE
    except Exception:  # noqa: BLE001
        return False


def _pick_cpu_threads():
    """The host side of a GPU box is not tuned for CPU inference: torch's default of 128 threads on the round-2 box ran HF Llama-7B
    at 0.66 tokens/s.  A baseline should be the best the host can do, so the thread count is chosen by a probe shaped like the work
    itself: a bf16 `F.linear` of one row against an 8192 x 8192 bf16 weight (128 MB, what a decoder Linear is), allocated under the
    interleaved policy, at 8 .. all cores (powers of two and the core count) — fastest wins.  Returns (threads, probe GB/s, table)."""
    import torch
    limit = len(os.sched_getaffinity(0))
    try:        # cgroup v2 CPU quota, if any
        quota, period = Path("/sys/fs/cgroup/cpu.max").read_text().split()
        if quota != "max":
            limit = max(1, min(limit, int(int(quota) / int(period))))
    except Exception:  # noqa: BLE001
        pass
    torch.set_num_threads(1)            # the allocating (first-touching) thread is this one: pages follow ITS memory policy
    w = torch.randn(8192, 8192).to(torch.bfloat16)
    x = torch.randn(1, 8192).to(torch.bfloat16)
    counts = sorted({n for n in (8, 16, 32, 64, 96, 128, 192, 256, limit) if n <= limit}) or [limit]
    best, best_t, table = None, 1e9, {}
    for n in counts:
        torch.set_num_threads(n)
        torch.nn.functional.linear(x, w)
        t0 = time.perf_counter()
        for _ in range(5):
            torch.nn.functional.linear(x, w)
        dt = (time.perf_counter() - t0) / 5
        table[n] = round(8192 * 8192 * 2 / dt / 1e9, 1)
        if dt < best_t:
            best, best_t = n, dt
    torch.set_num_threads(best or min(limit, 8))
    return torch.get_num_threads(), 8192 * 8192 * 2 / best_t / 1e9, table


def _masked_argmax(logits, banned):
    s = logits.float().clone()
    for i in banned:
        s[i] = float("-inf")
    return int(s.argmax()), s


def _teacher_forced_parity(step_fn, first_logits, device_tokens, banned, budget_s):
    """Greedy decode on the CPU, teacher-forced with the DEVICE's tokens: at every step the CPU's argmax is compared with
    the token the device produced.  A mismatch counts as a near-tie when the CPU's top-2 logits are within 2 bf16 ulps
    (two correct bf16 pipelines may order them either way).  Returns (tokens/s, identical, near_ties, compared)."""
    import torch
    logits, same, near, done = first_logits, 0, 0, 0
    t0 = time.perf_counter()
    for tok in device_tokens:
        mine, scores = _masked_argmax(logits, banned)
        if mine == tok:
            same += 1
        else:
            top2 = torch.topk(scores, 2)[0]
            near += int(float(top2[0] - top2[1]) <= 2 * float(top2[0].abs()) * 2.0 ** -7 + 1e-6)
        done += 1
        if done == len(device_tokens) or (time.perf_counter() - t0 > budget_s and done >= 2):
            break
        logits = step_fn(tok)
    steps = max(1, done - 1)        # forwards executed inside the timed region
    return steps / (time.perf_counter() - t0), same, near, done


def cpu_baseline(model, ids, px, device_tokens, banned, args):
    """cpu_baseline of the run's own configuration: weights copied back from the device (fp8: the de-quantised effective
    weights), prefix embeddings (ViT + projector + splice) from the oracle's glue, then
      * "reference": HF LlamaForCausalLM, bf16, KV cache — the reference's decode path (generate.py:218-227 ->
        v1/modeling_detikzify.py:218-283 -> HF LlamaModel) on the host cores;
      * "port": the oracle's LLaMA restatement (oracle/llama.py) on the same tensors.
    Both teacher-forced with the device's greedy tokens, which makes the baseline leg a token-parity check as well."""
    import torch
    from oracle.model import DetikzifyOracle
    from oracle.synth import tensor_specs
    t0 = time.perf_counter()
    cfg = model.config.oracle_dict()
    interleaved = _interleave_memory()
    torch.set_num_threads(1)            # the weights are first touched by THIS thread (whose policy is interleaved), not by a pool
    w = {}
    for name, shape, _, _ in tensor_specs(cfg):
        t = model.read_tensor(name).reshape(shape)
        keep_bf16 = t.dim() == 2 and name.startswith(("model.layers.", "lm_head"))     # decoder Linear weights: native bf16 GEMMs
        w[name] = t.clone() if keep_bf16 else t.float()
    t_copy = time.perf_counter() - t0
    threads, probe_gbs, table = _pick_cpu_threads()
    out = {"unit": "tokens/s", "cores": threads, "host_cpus": len(os.sched_getaffinity(0)), "memory_interleaved": interleaved,
           "thread_sweep_GBps": table,
           "thread_choice": f"{threads} threads: fastest of {min(table)}..{max(table)} on a bf16 F.linear probe (1 x 8192 against 8192 x 8192, "
                            f"{'NUMA-interleaved' if interleaved else 'local'} allocation): {probe_gbs:.0f} GB/s"}
    toks = [int(t) for t in device_tokens[:args.cpu_tokens]]
    with torch.no_grad():
        oracle = DetikzifyOracle(cfg, w, precision="bf16")
        t1 = time.perf_counter()
        emb = oracle.input_embeds(ids, px[0])                     # ViT + projector + splice on the CPU (oracle glue)
        t_glue = time.perf_counter() - t1
        # ---- the reference's engine
        hf = _hf_llama(cfg, w)
        t1 = time.perf_counter()
        res = hf(inputs_embeds=emb.to(torch.bfloat16)[None], use_cache=True)
        t_prefill = time.perf_counter() - t1
        state = {"kv": res.past_key_values}

        def hf_step(tok):
            r = hf(input_ids=torch.tensor([[tok]]), past_key_values=state["kv"], use_cache=True)
            state["kv"] = r.past_key_values
            return r.logits[0, -1]
        rate, same, near, n = _teacher_forced_parity(hf_step, res.logits[0, -1], toks, banned, args.cpu_budget)
        out.update(value=rate, kind="reference", parity_tokens_identical=f"{same}/{n}", parity_near_ties=near,
                   prefill_s=round(t_prefill, 2),
                   sample=f"{n - 1} greedy decode steps at context {ids.numel()}+ of the {cfg['layers']}-layer d={cfg['hidden']} decoder through "
                          f"the installed HuggingFace LlamaForCausalLM (transformers {__import__('transformers').__version__}, the class the "
                          f"reference subclasses) in bf16 with its KV cache on {threads} threads, same weights as the device (copied back, "
                          f"{t_copy:.0f} s, not timed), image prefix by the oracle's CPU glue (ViT + projector, {t_glue:.1f} s, not timed), "
                          f"prefill {t_prefill:.1f} s (not timed); teacher-forced with the device's greedy tokens")
        del hf, state, res
        # ---- the oracle port on the same tensors
        try:
            first = oracle.llm.logits(oracle.llm.forward(emb)[-1])
            rate, same, near, n = _teacher_forced_parity(lambda t: oracle.step(t), first, toks[:max(2, args.cpu_tokens // 2)],
                                                         banned, args.cpu_budget / 2)
            out["port"] = {"value": rate, "unit": "tokens/s", "cores": threads, "kind": "port", "parity_tokens_identical": f"{same}/{n}",
                           "parity_near_ties": near, "sample": f"{n - 1} steps of oracle/llama.py (bf16 rounding policy) on the same tensors"}
        except Exception as e:  # noqa: BLE001
            out["port"] = {"error": repr(e)}
    return out


def cpu_baseline_config1(budget_s):
    """BASELINE.json configs[0]: detikzify-ds-1.3b, one image, greedy decode on the CPU through the HuggingFace plumbing —
    LlamaForCausalLM at the ds-1.3b shape in fp32 with KV cache on seeded synthetic weights (no checkpoint offline), a
    243-position prefix, 64 greedy tokens."""
    import torch
    from detikzify_amd.model.config import preset
    cfg = preset("detikzify-ds-1.3b").oracle_dict()
    g = torch.Generator().manual_seed(1234)
    _interleave_memory()
    threads, probe_gbs, _ = _pick_cpu_threads()          # chosen for THIS entry, not inherited from whatever ran before
    t0 = time.perf_counter()
    d, ff, V, L = cfg["hidden"], cfg["ffn"], cfg["vocab"], cfg["layers"]

    def rnd(*shape):
        return (torch.randn(*shape, generator=g) * 0.02).to(torch.bfloat16)
    w = {"model.embed_tokens.weight": rnd(V, d), "lm_head.weight": rnd(V, d), "model.norm.weight": torch.ones(d, dtype=torch.bfloat16)}
    for i in range(L):
        p = f"model.layers.{i}."
        for n, s in (("self_attn.q_proj", (d, d)), ("self_attn.k_proj", (d, d)), ("self_attn.v_proj", (d, d)), ("self_attn.o_proj", (d, d)),
                     ("mlp.gate_proj", (ff, d)), ("mlp.up_proj", (ff, d)), ("mlp.down_proj", (d, ff))):
            w[p + n + ".weight"] = rnd(*s)
        w[p + "input_layernorm.weight"] = torch.ones(d, dtype=torch.bfloat16)
        w[p + "post_attention_layernorm.weight"] = torch.ones(d, dtype=torch.bfloat16)
    hf = _hf_llama(cfg, w).float()          # fp32 on the host, as BASELINE.md §3 specifies for config 1
    t_build = time.perf_counter() - t0
    prefix = (torch.randn(1, 243, d, generator=g) * 0.02)
    with torch.no_grad():
        t1 = time.perf_counter()
        res = hf(inputs_embeds=prefix, use_cache=True)
        t_prefill = time.perf_counter() - t1
        kv, logits, n = res.past_key_values, res.logits[0, -1], 0
        t1 = time.perf_counter()
        while n < 64 and (time.perf_counter() - t1 < budget_s or n < 2):
            r = hf(input_ids=logits.argmax().reshape(1, 1), past_key_values=kv, use_cache=True)
            kv, logits, n = r.past_key_values, r.logits[0, -1], n + 1
        dt = time.perf_counter() - t1
    return {"value": n / dt, "unit": "tokens/s", "cores": torch.get_num_threads(), "kind": "reference", "prefill_s": round(t_prefill, 2),
            "thread_choice": f"{threads} threads: fastest of 8..all cores on a bf16 F.linear probe ({probe_gbs:.0f} GB/s)",
            "sample": f"BASELINE config 1: HuggingFace LlamaForCausalLM at the ds-1.3b shape, fp32, KV cache, seeded synthetic weights "
                      f"(built in {t_build:.0f} s), 243-position prefix (prefill {t_prefill:.1f} s, not timed), {n} greedy tokens"}


def dump_outputs(dirname, sequences):
    """--dump-outputs: what the caller of the timed path received in its last step — model.generate's [1, prompt + new] token
    ids, stored as float64 (exact for token ids) so that two builds can be compared output for output"""
    import numpy as np
    d = Path(dirname)
    d.mkdir(parents=True, exist_ok=True)
    np.save(d / "sequences.npy", sequences.detach().cpu().numpy().astype(np.float64))


# ------------------------------------------------------------------------------------------------ main
def main():
    args = parse()
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    import torch
    import torch.distributed as dist
    import detikzify_amd.model as dmodel
    from detikzify_amd import dist as ddist
    from detikzify_amd.util import expand
    from detikzify_amd.util.synthetic import sketch_image

    if world != max(1, args.gpus):
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={world}: launch with torchrun --nproc-per-node {args.gpus} (one rank per GPU)")
    backend = os.environ.get("DTK_DIST_BACKEND", "nccl")     # "gloo": control-flow test of N ranks without N GPUs
    n_dev = max(1, torch.cuda.device_count())
    if world > 1:
        if local_rank >= n_dev and backend == "nccl":
            raise SystemExit(f"rank {rank}: local_rank {local_rank} but only {n_dev} GPUs")
        local_rank = local_rank % n_dev
        torch.cuda.set_device(local_rank)
        ddist.init_process_group(backend, timeout_s=1800)
        assert dist.get_backend() == backend and dist.get_world_size() == world
    red_dev = "cuda" if backend == "nccl" else "cpu"
    if world > 1 and backend == "nccl":
        ddist.pin_to_gpu_numa_node(local_rank)      # each rank's tree / reward threads stay on its GPU's NUMA node (DTK_NO_PIN=1: off)
    placement = ddist.gather_objects(ddist.placement())         # rank 0: who drives which GPU
    if rank == 0 and world > 1 and backend == "nccl":
        gpus = {(p.get("cuda_device"), p.get("pci_bus_id"), p.get("device_uuid")) for p in placement}
        assert len(gpus) == world, f"{world} ranks on {len(gpus)} distinct GPUs: {placement}"

    n_slots = min(64, args.batch) + min(8, max(1, args.batch_images)) if args.batch > 1 else 0   # + a prefix-cache slot per image (<= 8)
    model, proc = dmodel.load(args.model, synthetic=1234, device_map=local_rank, batch_slots=n_slots, weight_format=args.weight_format)
    model.reuse_prefix = bool(args.reuse)
    cfg = model.config
    img = sketch_image(0, 224)
    img = expand(img, max(img.size), do_trim=True)                 # P1 (host)
    enc = proc(images=img, return_tensors="pt")                    # P2/P3 (host): pixels resident before timing
    ids, px = enc.input_ids, enc.pixel_values
    T0 = ids.shape[1]
    n_new = args.new_tokens
    eos_ids = cfg.eos_token_id if isinstance(cfg.eos_token_id, (list, tuple)) else [cfg.eos_token_id]
    gen_kw = dict(pixel_values=px, bad_words_ids=[[cfg.image_token_id]], begin_suppress_tokens=list(eos_ids),
                  suppress_tokens=list(eos_ids), max_new_tokens=n_new, eos_token_id=-1)
    if args.sample:
        gen_kw.update(do_sample=True, temperature=0.8, top_p=0.95, top_k=0)
    else:
        gen_kw.update(do_sample=False)

    def rollout(i):
        out = model.generate(input_ids=ids, seed=1000 + rank + 7919 * i, **gen_kw)
        assert out.shape[1] == T0 + n_new
        return out

    def fence():
        model.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def max_over_ranks(seconds):
        if world == 1:
            return seconds
        t = torch.tensor([seconds], dtype=torch.float64, device=red_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    for i in range(args.warmup):
        rollout(-1 - i)
    fence()
    per_step, prefill_ms, vit_ms = [], [], []
    t0 = time.perf_counter()
    codes, first_tokens = [], None
    for i in range(args.steps):
        ts = time.perf_counter()
        out = rollout(i)
        toks = out[0, T0:]
        per_step.append(time.perf_counter() - ts)
        st = model.stats()
        prefill_ms.append(st["last_prefill_ms"]); vit_ms.append(st["last_vit_ms"])
        codes.append(proc.decode(toks, skip_special_tokens=True))
        if first_tokens is None:
            first_tokens = toks.tolist()
    if world > 1:   # the path's one exchange: finished TikZ strings to rank 0 (which scores them, eval.py:134-136)
        gathered = ddist.gather_objects(codes)
        assert (gathered is None) == (rank != 0) and (rank != 0 or len(gathered) == world)
    fence()
    elapsed = max_over_ranks(time.perf_counter() - t0)

    total_tokens = world * args.steps * n_new
    value = total_tokens / elapsed
    st = model.stats()
    W, Kb = st["weight_bytes_per_token"], st["kv_bytes_per_ctx_token"]
    mean_ctx = T0 + (n_new - 1) / 2.0
    bytes_per_token = W + Kb * mean_ctx
    dec_s = [s - p / 1e3 for s, p in zip(per_step, prefill_ms)]
    decode_tok_s = n_new / (sum(dec_s) / len(dec_s))
    result = {
        "metric": "tikz_tokens_per_sec", "value": value, "unit": "tokens/s", "n_gpus": world,
        "steps": args.steps, "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "bf16" if args.weight_format == "bf16" else "fp8-e4m3 weights / bf16 activations", "data": "synthetic",
        "config": {"workload": f"{args.model} (synthetic weights, seed 1234), 1 image 224x224->384x384, {T0}-token prefix, "
                               f"{'sampling T=.8 p=.95' if args.sample else 'greedy'} decode of {n_new} tokens per rollout, "
                               f"batch 1 per GPU, hipGraph per token" + (", image/prefix reuse" if args.reuse else ""),
                   "tokens_per_rollout": n_new, "prefix_tokens": T0, "rollouts_per_gpu": args.steps},
        "rollouts_per_sec": world * args.steps / elapsed,
        "decode_tokens_per_sec_per_gpu": decode_tok_s,
        "prefill_ms": sum(prefill_ms) / len(prefill_ms), "vit_ms": sum(vit_ms) / len(vit_ms),
        "decode_step": {"algorithmic_bytes_per_token": bytes_per_token, "achieved_GBps": bytes_per_token * decode_tok_s / 1e9,
                        "frac_of_hbm_peak": bytes_per_token * decode_tok_s / 1e9 / HBM_PEAK_GBS,
                        "roofline_tokens_per_sec": HBM_PEAK_GBS * 1e9 / bytes_per_token},
        "ranks": placement,
    }
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, out)
    if not args.full:
        if rank == 0:
            print(json.dumps(result), flush=True)
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()
        return
    # ---- the two MFMA-shaped stages of a rollout against THEIR rooflines (VERDICT r5 weak 10 / missing 5).  The decoder prefill at
    # M = 243 rows has an arithmetic intensity of ~243 FLOP/B, below the ~312 FLOP/B ridge of this part (2.5 PFLOP/s / 8 TB/s): its
    # floor is ONE pass over the decoder weights, i.e. HBM; the ViT (729 rows) is matrix-core bound.
    try:
        c = model.config
        n_p, D, mlp = (c.vit_image // c.vit_patch) ** 2, c.vit_dim, c.vit_mlp
        vit_flops = c.vit_depth * (2.0 * n_p * (4 * D * D + 2 * D * mlp) + 4.0 * n_p * n_p * D) + 2.0 * n_p * D * 3 * c.vit_patch ** 2
        p_ms, v_ms = result["prefill_ms"], result["vit_ms"]
        dec_ms = max(p_ms - v_ms, 1e-6)
        sec = {"decoder_prefill_ms": dec_ms, "prefill_rows": T0, "prefill_bound": "hbm",
               "prefill_bytes": W, "prefill_frac_of_hbm": W / (dec_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
               "vit_ms": v_ms, "vit_flops": vit_flops, "vit_bound": "mfma", "vit_peak_tflops": 2500.0,
               "vit_frac_of_mfma": vit_flops / (v_ms * 1e-3) / 2.5e15 if v_ms > 0 else None}
        try:        # MFMA-busy of the two GEMM kernels from the committed counter pass (a counter pass cannot run inside this process)
            busy = json.loads((ROOT / "profiles" / "mfma_busy.json").read_text())
            if busy.get("model") == args.model:
                sec["mfma_busy"] = busy
        except Exception:  # noqa: BLE001
            pass
        result["secondary_rooflines"] = sec
    except Exception as e:  # noqa: BLE001
        result["secondary_rooflines"] = {"error": repr(e)}

    # ---- B independent rollouts per GPU decoded as ONE batch (root-parallel trees of one GPU): the
    # weights are streamed once per step for all B sequences
    if args.batch > 1 and not args.skip_batched:
        import threading
        from detikzify_amd.infer.batching import make_engine
        engine = make_engine(model, max_batch=args.batch)      # the native run loop (DTK_ENGINE=python: the Python-driven engine)
        try:
            # MCTS rollouts sample with the pipeline's defaults (temperature .8, top-p .95: generate.py:362-364)
            mcts_kw = {**gen_kw, "do_sample": True, "temperature": 0.8, "top_p": 0.95, "top_k": 0}
            n_img = max(1, min(args.batch_images, args.batch))
            px_of = [px] + [proc(images=expand(sketch_image(100 + k, 224), 224, do_trim=True), return_tensors="pt").pixel_values
                            for k in range(1, n_img)]

            def one(i):
                model.generate(input_ids=ids, seed=5000 + rank * 100 + i, **{**mcts_kw, "pixel_values": px_of[i % n_img]})
            for rep_i in range(2):          # first pass warms the batch graph up
                fence()
                tb = time.perf_counter()
                engine.expect(args.batch)      # the B rollouts start together: first step once all have joined
                ths = [threading.Thread(target=one, args=(i,)) for i in range(args.batch)]
                [t.start() for t in ths]
                [t.join() for t in ths]
                fence()
                t_end = time.perf_counter()
                tb = t_end - tb
            est = engine.stats()
            tb = max_over_ranks(tb)
            # HBM bytes one step must move: the weights once, every slot's PRIVATE keys (its generated tokens), and the image
            # prefix once per image — forked slots read the prefix rows from their source slot (share_prefix_reads), so it is
            # not B copies.  (SURVEY §8d's formula W + sum_b K*t_b counts it B times: kept as frac_of_survey_formula.)
            bytes_survey = W + args.batch * Kb * mean_ctx
            shared = T0 if engine.share_prefix else 0
            bytes_step = W + args.batch * Kb * (mean_ctx - shared) + n_img * Kb * shared
            result["batched_rollouts"] = {
                "batch_per_gpu": args.batch, "images_in_flight": n_img, "prefix_encodes_both_passes": engine.prefix_encodes,
                "rollouts_per_sec": world * args.batch / tb,
                "tokens_per_sec": world * args.batch * n_new / tb, "ms_per_batch": 1e3 * tb,
                "decode_steps": est["steps"], "algorithmic_bytes_per_step": bytes_step,
                # one lock-step decode step per generated token; joins / forks / host time are inside tb, so this is the
                # end-to-end fraction of the decode-step HBM roofline (W once per step + every sequence's own KV)
                "achieved_GBps": bytes_step * n_new / tb / 1e9,
                "frac_of_hbm_peak": bytes_step * n_new / tb / 1e9 / HBM_PEAK_GBS,
                "roofline_rollouts_per_sec": world * args.batch * HBM_PEAK_GBS * 1e9 / (bytes_step * n_new),
                "frac_of_survey_formula": bytes_survey * n_new / tb / 1e9 / HBM_PEAK_GBS,
                "survey_formula_bytes_per_step": bytes_survey,
                "bytes_note": "algorithmic_bytes_per_step = W + B*K*(mean context - prefix) + images*K*prefix: the shared image prefix is read once "
                              "per image, not once per slot; frac_of_survey_formula keeps SURVEY 8d's W + sum_b K*t_b (rounds 1-2 quoted that)",
                "prefix_sharing": bool(engine.share_prefix),
                "engine": est,      # both passes
                "decode": f"sampling T=.8 top_p=.95 (DetikzifyPipeline defaults), {n_new} tokens, EOS suppressed",
                "note": "B independent rollouts (own KV slot, seed) per GPU through model.generate from B threads; one "
                        f"dtk_decode_batch step serves all of them; the {T0}-token image prefix is encoded once, its KV "
                        "forked into each slot (bit-identical to a full prefill, SURVEY f1) and read from one copy"}
        except Exception as e:  # noqa: BLE001
            result["batched_rollouts"] = {"error": repr(e)}
        finally:
            engine.close()

    # ---- the MCTS metric: the search itself (detikzify_amd.infer: DetikzifyGenerator per tree, reference semantics)
    trees = min(args.batch, 64) if args.mcts_trees < 0 else min(args.mcts_trees, max(args.batch, 0))
    want_c4 = not args.no_config4 and args.batch >= 2
    want_c5 = not args.no_config5
    if args.mcts_seq_expansions > 0 or trees > 1 or want_c4 or want_c5 or args.reward_latency:
        from detikzify_amd.infer import DetikzifyPipeline, SyntheticTikzDocument
        from detikzify_amd.infer.batching import simulate_parallel_images
        mcts = {"reward": "SelfSim (device ViT, reference-image features cached) of SyntheticTikzDocument renderings — LaTeX is absent "
                          "offline: stub-reward numbers, not comparable with real-LaTeX runs",
                "max_length": T0 + n_new, "sampling": "temperature .8, top-p .95 (DetikzifyPipeline defaults)",
                "roofline_note": "frac_of_roofline = generated tokens/s over what the decode-step HBM roofline allows a batch of that many "
                                 "slots: b * 8 TB/s / (W + b*K*n_new/2 + images*K*prefix) — the weights once per step, every slot's own "
                                 "keys at the mean depth of a from-the-root rollout, the image prefix once per image"}

        def search(the_model, the_proc, images, trees_per_image, expansions, ragged=False, pipe_kw=None, Wk=None, slots=None):
            """This rank's share of a root-parallel search: len(images) * trees_per_image trees as ONE batched decode (one tree:
            the unmodified sequential search), then the path's single exchange — (score, code) records to rank 0 — timed on its
            own.  Every rank calls this (the gather is a collective) even with no image of its own."""
            base = ragged_pipeline_class(DetikzifyPipeline, n_new) if ragged else DetikzifyPipeline
            pipe = base(the_model, the_proc, **{**dict(metric="model", document_class=SyntheticTikzDocument, max_length=T0 + n_new),
                                                **(pipe_kw or {})})
            if getattr(pipe, "metric", None) is not None and hasattr(pipe.metric, "cache_reference"):
                pipe.metric.cache_reference = True           # f1: a reference image's features are computed once
            n_trees = len(images) * trees_per_image
            s0 = the_model.stats()
            fence()
            t_begin = time.perf_counter()
            local = [[] for _ in images]
            if n_trees:
                for k, score, doc in simulate_parallel_images(pipe, images, trees_per_image, expansions, slots=slots,
                                                              seeds=[ddist.tree_seed(1000, t) for t in range(n_trees)]):
                    local[k].append([float(score), doc.code])
            t_search = time.perf_counter() - t_begin
            t_g = time.perf_counter()
            gathered = ddist.gather_objects([len(images), sum(len(x) for x in local), t_search, local])
            t_gather = time.perf_counter() - t_g
            fence()
            total_s = max_over_ranks(time.perf_counter() - t_begin)
            s1 = the_model.stats()
            eng = (getattr(the_model, "last_batch_stats", None) or {}) if n_trees > 1 else {}
            tokens = eng.get("tokens_out") if n_trees > 1 else None
            out = {"trees_per_gpu": n_trees, "images_per_gpu": len(images), "expansions_per_tree": expansions, "ragged_lengths": bool(ragged),
                   "seconds": total_s, "search_seconds_this_rank": round(t_search, 3), "gather_seconds": round(max_over_ranks(t_gather), 4),
                   "decode_steps_per_gpu": (eng.get("steps") if n_trees > 1 else s1["decode_steps"] - s0["decode_steps"]),
                   "tokens_generated_per_gpu": tokens, "vit_passes_per_gpu": s1["vit_images"] - s0["vit_images"]}
            if n_trees > 1:
                out["engine"] = eng
            if gathered is not None:            # rank 0: the whole job
                n_roll = sum(g[1] for g in gathered)
                rates = [g[1] / g[2] for g in gathered if g[2] > 0 and g[1] > 0]
                out.update(rollouts=n_roll, rollouts_per_sec=n_roll / total_s,
                           per_rank_rollouts_per_sec_min_max=[round(min(rates), 3), round(max(rates), 3)] if rates else None,
                           merged_on_rank0=sum(len(ddist.merge_rollouts([img])) for g in gathered for img in g[3]))
                scores = [r[0] for g in gathered for img in g[3] for r in img]
                out["scores_min_max"] = [min(scores), max(scores)] if scores else None
                if Wk is not None and tokens and n_trees > 1:
                    Wm, Km = Wk
                    nb = min(n_trees, slots) if slots else n_trees          # decode slots in use
                    roof = nb * HBM_PEAK_GBS * 1e9 / (Wm + nb * Km * n_new / 2.0 + len(images) * Km * T0)
                    out.update(tokens_per_sec_this_gpu=tokens / t_search, roofline_tokens_per_sec_per_gpu=roof,
                               frac_of_roofline=tokens / t_search / roof)
            return out

        img0 = sketch_image(0, 224)
        try:
            if args.mcts_seq_expansions > 0:
                # ONE tree per GPU: the unmodified sequential search (selection k+1 depends on back-propagation k); over N ranks
                # this is root parallelisation with seeds 1000 + rank
                r = search(model, proc, [img0], 1, args.mcts_seq_expansions)
                steps = r["decode_steps_per_gpu"]
                r["frac_of_hbm_peak"] = steps * (W + Kb * T0) / r["seconds"] / 1e9 / HBM_PEAK_GBS
                r["roofline_rollouts_per_sec_at_512_tokens"] = world * HBM_PEAK_GBS * 1e9 / (bytes_per_token * n_new)
                mcts["sequential"] = r
            if trees > 1:
                mcts["parallel"] = search(model, proc, [img0], trees, args.mcts_expansions, Wk=(W, Kb))
                if args.mcts_oversubscribe > 1:
                    # more trees than decode slots: a tree holds a slot only while it generates, so the reward waves of one part of the
                    # trees are covered by the decoding of the others (with fixed-length rollouts every tree of a batch reaches its
                    # reward on the same step — the 64-tree run above idles there)
                    mcts["parallel_oversubscribed"] = search(model, proc, [img0], int(trees * args.mcts_oversubscribe), args.mcts_expansions,
                                                             Wk=(W, Kb), slots=trees)
                    mcts["parallel_oversubscribed"]["decode_slots"] = trees
            if want_c4:
                # BASELINE configs[3]: "ds-7b, MCTS refine (16 rollouts, LaTeX-compile reward) sharded across 8 MI355X" — 16 rollouts of ONE
                # image in total: rank r grows shard_expansions(16, N)[r] trees of one expansion each as one batch (N=1: 16 trees,
                # N=8: 2 per rank; reference examples/eval.py:108-137 is the per-image loop this shards)
                mine = ddist.shard_expansions(16, world)[rank]
                # a context of the size this rank's share needs (trees + one prefix-cache slot: load(batch_slots = rollouts + images),
                # what a caller of this configuration would load) — the kernels a context decodes with follow ITS size (2 / 4 trees: the
                # multi-vector family; 8 / 16: one MFMA column tile with the per-slot attention walk), not the 65-slot batch's above
                n4 = min(mine, args.batch)
                t_l = time.perf_counter()
                slots4 = 5 if n4 <= 4 else n4 + 1           # <= 4 trees: the 5-slot context of the multi-vector family (what rank_shape's N = 4 / 8 blocks load)
                c4_model, c4_proc, load_error = model, proc, None
                if 1 <= n4 and slots4 < model.num_slots():
                    try:
                        c4_model, c4_proc = dmodel.load(args.model, synthetic=1234, device_map=local_rank, batch_slots=slots4, weight_format=args.weight_format)
                    except Exception as e:  # noqa: BLE001  (the searches below end in collectives: a rank without its own context decodes in the batch's)
                        load_error = repr(e)
                        print(f"[rank {rank}] config 4: no context of {slots4} slots ({load_error}); using the {model.num_slots()}-slot one", file=sys.stderr, flush=True)
                c4 = {"shape": "16 rollouts of one image over all ranks, root-parallel: 16/N trees x 1 expansion per rank",
                      "context_slots": c4_model.num_slots(), "context_load_seconds": round(time.perf_counter() - t_l, 1), "context_load_error": load_error,
                      "fixed_length": search(c4_model, c4_proc, [img0] if mine else [], n4, 1, Wk=(W, Kb)),
                      "ragged": search(c4_model, c4_proc, [img0] if mine else [], n4, 1, ragged=True, Wk=(W, Kb))}
                if world == 1 and not args.no_rank_shapes:
                    # What rank 0 of an N-GPU job would decode, run here on ONE GPU: 16/N trees of one expansion (N = 4 / 8: 4 / 2
                    # trees in a 5-slot context = the multi-vector kernels; N = 2: 8 trees = one MFMA column tile).  Every rank of
                    # such a job has the same shape and the path has no data-path collective (one gather of strings at the end), so
                    # N x this rank's rate is what the N-GPU job should deliver; SCALE_rNN.json then only has to confirm it.
                    shapes, small, m_, p_ = {}, None, None, None
                    try:
                        for N in (2, 4, 8):
                            per = ddist.shard_expansions(16, N)[0]
                            if per <= 4 and small is None:
                                t_l = time.perf_counter()
                                small = dmodel.load(args.model, synthetic=1234, device_map=local_rank, batch_slots=5, weight_format=args.weight_format)
                                shapes["small_context_load_seconds"] = round(time.perf_counter() - t_l, 1)
                            m_, p_ = small if per <= 4 else (c4_model, c4_proc)
                            per = per if per <= 4 else min(per, args.batch)
                            r = search(m_, p_, [img0], per, 1, Wk=(W, Kb))
                            rate = r.get("rollouts_per_sec")
                            shapes[f"N{N}"] = {"trees_per_rank": per, "context_slots": m_.num_slots(),
                                               "step_kernels_cover_slots": m_.stats().get("last_batch_step_slots"),
                                               "rollouts_per_sec_one_rank": rate, "predicted_rollouts_per_sec_at_N": None if rate is None else N * rate,
                                               "predicted_scaling_vs_N1": None if not (rate and c4["fixed_length"].get("rollouts_per_sec")) else
                                               N * rate / c4["fixed_length"]["rollouts_per_sec"],
                                               "seconds": r["seconds"], "decode_steps": r["decode_steps_per_gpu"], "frac_of_roofline": r.get("frac_of_roofline"),
                                               "ms_per_decode_step": (1e3 * (r.get("engine") or {}).get("wait_s", 0.0) / r["decode_steps_per_gpu"]) if r.get("decode_steps_per_gpu") else None}
                    finally:
                        if small is not None:
                            del small, m_, p_
                            import gc
                            gc.collect()
                    c4["rank_shape"] = shapes
                if c4_model is not model:
                    del c4_model, c4_proc
                    import gc
                    gc.collect()
                mcts["config4"] = c4
            for S in args.reward_latency:
                # f3: what a reward that costs what LaTeX costs does to rollouts/s.  The renderer sleeps S seconds per document
                # (DTK_SYNTH_COMPILE_SECONDS) either in the tree's own thread (pool off: what TikzDocument's subprocess call does
                # to a tree) or in a CompilePool worker process (pool on); ragged rollout lengths so rewards do not all start at
                # the same step.  Reference: examples/refine.py:151-185 (pool + imap), infer/tikz.py:89-147 (1-60 s per document).
                from detikzify_amd.infer.compile_pool import CompilePool, pooled_document_class
                from detikzify_amd.infer.tikz import SleepingSyntheticTikzDocument
                os.environ["DTK_SYNTH_COMPILE_SECONDS"] = str(S)
                entry = {}
                # the last variant runs TWICE as many trees as there are decode slots (pool on): a tree that waits for its compile
                # holds no slot, so the other half decodes meanwhile — what hides a reward of seconds when one batch of trees cannot
                for n_t, over in ((1, False), (trees, False), (2 * trees, True)) if trees > 1 else ((1, False),):
                    for pooled in ((True,) if over else (False, True)):
                        pool = CompilePool(workers=min(128, max(1, n_t)), document_class=SleepingSyntheticTikzDocument) if pooled else None
                        try:
                            if pool is not None:
                                pool.warm()
                            doc_cls = pooled_document_class(pool) if pooled else SleepingSyntheticTikzDocument
                            r = search(model, proc, [img0], n_t, 2, ragged=True, pipe_kw=dict(document_class=doc_cls), Wk=None if over else (W, Kb),
                                       slots=trees if over else None)
                        finally:
                            if pool is not None:
                                pool.close()
                        busy = (r.get("engine") or {}).get("wait_s")
                        entry[f"{n_t}_trees_over_{trees}_slots_pool_on" if over else f"{n_t}_trees_pool_{'on' if pooled else 'off'}"] = {
                            k: r.get(k) for k in ("rollouts", "rollouts_per_sec", "seconds", "decode_steps_per_gpu", "tokens_generated_per_gpu",
                                                  "frac_of_roofline")} | {"engine_wait_s": busy}
                mcts.setdefault("reward_latency", {})[f"{S:g}s"] = entry
                os.environ.pop("DTK_SYNTH_COMPILE_SECONDS", None)
        except Exception as e:  # noqa: BLE001
            mcts["error"] = repr(e)
        if want_c5:
            # BASELINE configs[4]: "cl-7b fp8 weights, batch=8 images, MCTS 32 rollouts on 8 MI355X": the images are striped over the
            # ranks (images[r::N], exact reference sharding, examples/eval.py:80-83), every image gets --config5-trees trees x
            # --config5-expansions expansions = 32 rollouts, all of a rank's trees decode as ONE batch, one gather to rank 0.
            # N=1: 8 images x 8 trees = 64 slots + 8 prefix-cache slots on one GPU; N=8: one image, 8 slots per GPU.
            try:
                imgs5 = [sketch_image(200 + k, 224) for k in range(args.config5_images)]
                mine5 = ddist.chunk(list(range(len(imgs5))), world)[rank]
                slots5 = len(mine5) * args.config5_trees
                t_load = time.perf_counter()
                # the searches below end in collectives: a rank whose model does not load (e.g. no memory) must take every other rank
                # out of this block with it, not leave them waiting in a gather — the ranks agree on the outcome first
                m5 = p5 = load_error = None
                try:
                    m5, p5 = dmodel.load(args.config5_model, synthetic=1234, device_map=local_rank, weight_format="fp8",
                                         batch_slots=max(2, min(64, slots5) + min(8, max(1, len(mine5)))))
                except Exception as e:  # noqa: BLE001
                    load_error = repr(e)
                failed = [(r, err) for r, err in enumerate(ddist.gather_objects(load_error, all_ranks=True)) if err]
                if failed:
                    del m5, p5
                    raise RuntimeError(f"{args.config5_model} did not load on rank(s) {[r for r, _ in failed]}: {failed[0][1]}")
                t_load = time.perf_counter() - t_load
                st5 = m5.stats()
                Wk5 = (st5["weight_bytes_per_token"], st5["kv_bytes_per_ctx_token"])
                c5 = {"shape": f"{args.config5_model} fp8 weights, {len(imgs5)} images striped over the ranks, {args.config5_trees} trees x "
                               f"{args.config5_expansions} expansions = {args.config5_trees * args.config5_expansions} rollouts per image",
                      "model_load_seconds": round(t_load, 1), "weight_bytes_per_token": Wk5[0]}
                try:
                    for key, ragged in (("fixed_length", False), ("ragged", True)):
                        c5[key] = search(m5, p5, [imgs5[i] for i in mine5], args.config5_trees, args.config5_expansions, ragged=ragged, Wk=Wk5)
                    # 0 = the default since round 5: bf16 activations (fp8 weights widened in registers, bf16 MFMA).  MXFP8 activations on
                    # the fp8 matrix cores (v_mfma_scale_f32_16x16x128_f8f6f4, csrc/kernels_batch_mx.hip) are OPT-IN (dtk_set_option act_fp8 = 1 /
                    # DTK_OPTIONS=act_fp8=1): they move the logits ~1e-1 rel-L2 (tests/test_gpu_parity_batched.py::
                    # test_mxfp8_activations_against_bf16_activations asserts and prints the figures), so the faster step is the caller's choice
                    c5["decode_steps_on_fp8_matrix_cores"] = int(m5.stats().get("last_batch_step_fp8_mfma", 0))
                    try:
                        m5.set_option("act_fp8", 1)
                        c5["fixed_length_fp8_matrix_cores_opt_in"] = search(m5, p5, [imgs5[i] for i in mine5], args.config5_trees, args.config5_expansions, Wk=Wk5)
                        c5["fixed_length_fp8_matrix_cores_opt_in"]["decode_steps_on_fp8_matrix_cores"] = int(m5.stats().get("last_batch_step_fp8_mfma", 0))
                    finally:
                        m5.set_option("act_fp8", 0)
                    if world == 1 and not args.no_rank_shapes:
                        # one rank's share at N = 2 / 4 / 8: 8/N images x the same trees (32 / 16 / 8 decode slots: two / one MFMA
                        # column tiles — the kernels a step runs follow its highest active slot, so the 72-slot context runs
                        # exactly what an N-GPU rank's smaller context would)
                        shapes5 = {}
                        for N in (2, 4, 8):
                            imgs_n = ddist.chunk(list(range(len(imgs5))), N)[0]
                            r = search(m5, p5, [imgs5[i] for i in imgs_n], args.config5_trees, args.config5_expansions, Wk=Wk5)
                            rate = r.get("rollouts_per_sec")
                            shapes5[f"N{N}"] = {"images_per_rank": len(imgs_n), "trees_per_rank": len(imgs_n) * args.config5_trees,
                                                "step_kernels_cover_slots": m5.stats().get("last_batch_step_slots"),
                                                "rollouts_per_sec_one_rank": rate, "predicted_rollouts_per_sec_at_N": None if rate is None else N * rate,
                                                "predicted_scaling_vs_N1": None if not (rate and c5["fixed_length"].get("rollouts_per_sec")) else
                                                N * rate / c5["fixed_length"]["rollouts_per_sec"],
                                                "seconds": r["seconds"], "frac_of_roofline": r.get("frac_of_roofline")}
                        c5["rank_shape"] = shapes5
                finally:
                    del m5
                    import gc
                    gc.collect()
                mcts["config5"] = c5
            except Exception as e:  # noqa: BLE001
                import traceback
                print(f"[rank {rank}] mcts.config5 failed: {e!r}\n{traceback.format_exc()}", file=sys.stderr, flush=True)     # (only rank 0's line is printed)
                mcts["config5"] = {"error": repr(e)}
        result["mcts"] = mcts
        result["mcts_rollouts_per_sec"] = (mcts.get("parallel") or {}).get("rollouts_per_sec")
        result["mcts_rollouts_per_sec_sequential"] = (mcts.get("sequential") or {}).get("rollouts_per_sec")
        result["mcts_rollouts_per_sec_oversubscribed"] = (mcts.get("parallel_oversubscribed") or {}).get("rollouts_per_sec")
        result["mcts_config4_rollouts_per_sec"] = ((mcts.get("config4") or {}).get("fixed_length") or {}).get("rollouts_per_sec")
        result["mcts_config5_rollouts_per_sec"] = ((mcts.get("config5") or {}).get("fixed_length") or {}).get("rollouts_per_sec")
        result["mcts_config5_rollouts_per_sec_fp8_matrix_cores_opt_in"] = ((mcts.get("config5") or {}).get("fixed_length_fp8_matrix_cores_opt_in") or {}).get("rollouts_per_sec")
        for key in ("config4", "config5"):      # {N: predicted whole-job rollouts/s} from the one-rank shapes measured above
            rs = (mcts.get(key) or {}).get("rank_shape") or {}
            if rs:
                result[f"mcts_{key}_predicted_rollouts_per_sec"] = {k: v.get("predicted_rollouts_per_sec_at_N") for k, v in rs.items() if isinstance(v, dict)}

    if rank == 0:
        # ---- roofline of the dominant kernel: probe pass (plain launches, HIP events around the kernel)
        roof = {"bound": "hbm", "kernel": "k_gemv<PRO_RMSNORM,EPI_SWIGLU> (post_attention_layernorm + gate/up GEMV + SiLU*mul)",
                "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": None, "traffic": None}
        try:
            model.set_graph_mode(2)
            before = model.stats()
            model.generate(input_ids=ids, **{**gen_kw, "max_new_tokens": args.probe_tokens})
            after = model.stats()
            model.set_graph_mode(1)
            n = after["probe_kernel_launches"] - before["probe_kernel_launches"]
            ms = after["probe_kernel_ms_sum"] - before["probe_kernel_ms_sum"]
            if n > 0 and ms > 0:
                # `achieved` uses the RAW interval between the two events (conservative: an event pair with nothing in
                # between already reads empty_event_pair_us on this stream; rocprofv3's start->end for the same kernel —
                # rocprofv3_avg_us below, from the committed kernel-trace summary — is shorter than the interval)
                pair_ms = float(after.get("probe_event_pair_ms", 0.0) or 0.0)
                avg_ms = ms / n
                ach = after["probe_kernel_bytes"] / (avg_ms * 1e-3) / 1e9
                roof.update(achieved=ach, frac=ach / HBM_PEAK_GBS, avg_launch_us=avg_ms * 1e3, empty_event_pair_us=pair_ms * 1e3,
                            bytes_per_launch=after["probe_kernel_bytes"], launches_timed=n)
        except Exception as e:  # noqa: BLE001  (the bench line must still be printed)
            roof["error"] = repr(e)
            model.set_graph_mode(1)
        # second live measurement, the one `achieved` is quoted on: the SAME kernel launched back to back over all layers'
        # weights (distinct 180 MB per launch: nothing comes from L2 / Infinity Cache) between ONE pair of HIP events on the
        # library's stream — average launch duration including the kernel boundary, without the ~4.6 us an event pair
        # around every single launch adds (kept above as in_step_event_pair_us); this is the figure that has to agree with
        # rocprofv3's average for the kernel
        try:
            import ctypes as C
            us = C.c_float(0.0)
            model._check(model.lib.dtk_bench_gemv(model._ctx, 2, 0xFF, args.probe_chain_reps, C.byref(us)), "dtk_bench_gemv")
            if us.value > 0 and roof.get("bytes_per_launch"):
                ach = roof["bytes_per_launch"] / (us.value * 1e-6) / 1e9
                roof.update(in_step_event_pair_us=roof.get("avg_launch_us"), in_step_achieved=roof.get("achieved"),
                            achieved=ach, frac=ach / HBM_PEAK_GBS, avg_launch_us=float(us.value),
                            launches_timed=args.probe_chain_reps * cfg.layers,
                            method="HIP events around a back-to-back chain of this kernel over every layer's weights on the library's stream")
        except Exception as e:  # noqa: BLE001
            roof["chain_error"] = repr(e)
        # HBM traffic of that kernel: a counter pass cannot run inside this process, so the figure comes from the committed
        # rocprofv3 --pmc FETCH_SIZE summary (x2 gfx950 correction, guides/MI355X_MICROARCH.md §HBM) — but only while it
        # describes THIS kernel: profiles/dominant_kernel.json records the model and the sha256 of kernels_decode.hip it was
        # measured on; any other source or model reports null instead of a stale number
        try:
            meta = json.loads((ROOT / "profiles" / "dominant_kernel.json").read_text())
            sha = hashlib.sha256(DOMINANT_KERNEL_SOURCE.read_bytes()).hexdigest()
            if meta.get("model") == args.model and meta.get("weight_format", "bf16") == args.weight_format and meta.get("source_sha256") == sha:
                roof["traffic"] = meta["hbm_read_bytes_per_launch"]
                roof["traffic_source"] = meta["traffic_source"]
                roof["rocprofv3_avg_us"] = meta["rocprofv3_avg_us"]
                if roof.get("bytes_per_launch"):
                    roof["frac_at_rocprofv3_duration"] = roof["bytes_per_launch"] / (meta["rocprofv3_avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS
            else:
                roof["traffic_source"] = "none: profiles/dominant_kernel.json was measured on another model / kernel source"
        except Exception:  # noqa: BLE001
            pass
        result["roofline"] = roof
        if world == 1 and not args.no_cpu_baseline:
            banned = [cfg.image_token_id, *eos_ids]
            try:
                result["cpu_baseline"] = cpu_baseline(model, ids[0], px, first_tokens, banned, args)
            except Exception as e:  # noqa: BLE001
                result["cpu_baseline"] = {"value": None, "unit": "tokens/s", "cores": None, "kind": "reference", "sample": f"failed: {e!r}"}
            if not args.no_cpu_config1:
                try:
                    result["cpu_baseline"]["config1_ds1.3b_cpu"] = cpu_baseline_config1(args.cpu_budget)
                except Exception as e:  # noqa: BLE001
                    result["cpu_baseline"]["config1_ds1.3b_cpu"] = {"error": repr(e)}
        print(json.dumps(result), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
