"""Timing probe for the batched MCTS (search/mcts.py, ops/csrc/mcts.hip).

Run on a GPU box:

  python tools/mcts_probe.py search   one mcts_search, fused kernels against the
                                      torch step functions (STOIX_FUSED_MCTS=0)
                                      alternating in one process, and the two
                                      kernels alone
  python tools/mcts_probe.py sps      default ff_az and ff_sampled_az update
                                      steps, each setting in a fresh child
                                      process; prints steps per second
  python tools/mcts_probe.py count    three searches at the default ff_az point,
                                      to be run under
                                      `rocprofv3 --kernel-trace --stats` once per
                                      STOIX_FUSED_MCTS setting
  python tools/mcts_probe.py gate     the AlphaZero learning gate's configuration
                                      (tests/test_systems_e2e.py), fused path

Wall times are graph-free: a host clock around work that ends in a device
synchronise, and device events for the single kernels.
"""
from __future__ import annotations

import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

# (B, A, S): the default ff_az composition (1024 CartPole envs, 25 simulations)
# and a wider, deeper point
POINTS = [(1024, 2, 25), (1024, 18, 50)]
OBS, HID = 4, 64


def make_model(A, device):
    """A small fixed MLP world model + actor/critic as ``recurrent_fn``."""
    g = torch.Generator(device=device).manual_seed(A)
    r = lambda *s: torch.randn(*s, device=device, generator=g) / s[0] ** 0.5
    w_dyn, e_act = r(OBS, OBS), 0.5 * r(A, OBS)
    w1, w2, w_pi, w_v = r(OBS, HID), r(HID, HID), r(HID, A), r(HID, 1)

    def heads(obs):
        h = torch.tanh(torch.tanh(obs @ w1) @ w2)
        return h @ w_pi, (h @ w_v).squeeze(-1)

    def recurrent_fn(embedding, action):
        obs = torch.tanh(embedding["obs"] @ w_dyn + e_act[action])
        logits, value = heads(obs)
        discount = torch.full_like(value, 0.99)
        return {"obs": obs}, obs[:, 0], discount, logits, value

    return heads, recurrent_fn


def make_search(B, A, S, device):
    from stoix_amd.search.mcts import mcts_search

    heads, recurrent_fn = make_model(A, device)
    obs = torch.randn(B, OBS, device=device, generator=torch.Generator(device=device).manual_seed(1))
    logits, value = heads(obs)
    gen = torch.Generator(device=device).manual_seed(2)

    def search():
        return mcts_search(obs, {"obs": obs}, logits, value, recurrent_fn, S, generator=gen)

    return search


def wall_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def event_us(fn, iters=200, warmup=20):
    for _ in range(warmup):
        fn()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters * 1e3


def search_probe():
    from stoix_amd import ops
    from stoix_amd.search import mcts

    ops.ext(required=True)
    device = torch.device("cuda:0")
    for B, A, S in POINTS:
        search = make_search(B, A, S, device)
        times = {"1": [], "0": []}
        for rep in range(3):  # alternate the two settings
            for knob in ("1", "0"):
                os.environ["STOIX_FUSED_MCTS"] = knob
                times[knob].append(wall_ms(search, iters=3 if knob == "0" else 10, warmup=1))
        os.environ["STOIX_FUSED_MCTS"] = "1"
        fmt = lambda v: " / ".join(f"{x:.2f}" for x in v)
        print(f"mcts_search B={B} A={A} S={S}: fused {fmt(times['1'])} ms"
              f"  torch {fmt(times['0'])} ms  ratio {min(times['0']) / min(times['1']):.1f}x", flush=True)

        # the two kernels alone, on a tree of S - 1 expanded nodes: the last
        # simulation's descent, and its expansion + backup repeated in place
        heads, recurrent_fn = make_model(A, device)
        obs = torch.randn(B, OBS, device=device)
        logits, value = heads(obs)
        arena, emb_arena = mcts._new_search({"obs": obs}, torch.softmax(logits, -1), value, S)
        mcts._run_simulations(arena, emb_arena, recurrent_fn, S - 1, 1.25)
        sp, sa = mcts._select_hip(arena, S, 1.25)
        depth = torch.zeros(B, S + 1, dtype=torch.long, device=device)
        for s in range(1, S):
            depth[:, s] = depth[arena.batch, arena.parent[:, s]] + 1
        prior_new = torch.softmax(logits, -1)
        t_sel = event_us(lambda: mcts._select_hip(arena, S, 1.25))
        t_bak = event_us(lambda: mcts._expand_backup_hip(arena, S, sp, sa, value, value, prior_new, value))
        print(f"  kernels alone at sim {S} (mean selected depth {depth[arena.batch, sp].float().mean():.1f},"
              f" max {int(depth.max())}): mcts_select {t_sel:.1f} us  mcts_expand_backup {t_bak:.1f} us"
              " (eager launch to launch)", flush=True)


SYSTEMS = {
    "ff_az": ("stoix_amd.systems.search.ff_az", "default/anakin/default_ff_az.yaml"),
    "ff_sampled_az": ("stoix_amd.systems.search.ff_sampled_az", "default/anakin/default_ff_sampled_az.yaml"),
}


def sps_child(name, updates):
    """Default composition of one search system: update steps per second."""
    import importlib

    from stoix_amd import envs as environments
    from stoix_amd.config import compose
    from stoix_amd.utils.total_timestep_checker import check_total_timesteps

    module, default = SYSTEMS[name]
    cfg = compose(default, ["arch.total_timesteps=null", f"arch.num_updates={updates + 1}",
                            "arch.num_evaluation=1", "logger.loggers=[]"])
    cfg.arch.n_devices = 1
    check_total_timesteps(cfg)
    device = torch.device("cuda:0")
    torch.manual_seed(int(cfg.arch.seed))
    num_envs = int(cfg.arch.num_envs)
    env = environments.make_single(cfg, num_envs, device, seed=int(cfg.arch.seed))
    learner = importlib.import_module(module).learner_factory(cfg, env, device)
    ms = wall_ms(learner.update_step, iters=updates, warmup=1)
    steps = int(cfg.system.rollout_length) * num_envs
    print(json.dumps({"system": name, "fused": os.environ.get("STOIX_FUSED_MCTS", "1") != "0",
                      "num_envs": num_envs, "num_simulations": int(cfg.system.num_simulations),
                      "ms_per_update": round(ms, 1), "sps": round(steps / ms * 1e3)}), flush=True)


def sps_probe(updates=3):
    for name in SYSTEMS:
        for knob in ("1", "0", "1", "0"):
            env = dict(os.environ, STOIX_FUSED_MCTS=knob)
            subprocess.run([sys.executable, os.path.abspath(__file__), "_sps_child", name, str(updates)],
                           env=env, check=True, timeout=600)


def count_probe():
    B, A, S = POINTS[0]
    search = make_search(B, A, S, torch.device("cuda:0"))
    for _ in range(3):
        search()
    torch.cuda.synchronize()
    print(f"3 searches at B={B} A={A} S={S}, STOIX_FUSED_MCTS={os.environ.get('STOIX_FUSED_MCTS', '1')}")


def gate_probe():
    from stoix_amd.config import compose
    from stoix_amd.systems.search.ff_az import run

    cfg = compose(
        "default/anakin/default_ff_az.yaml",
        ["env=debug/identity", "arch.total_num_envs=32",
         "arch.total_timesteps=null", "arch.num_updates=40",
         "arch.num_evaluation=1", "arch.num_eval_episodes=16",
         "arch.absolute_metric=false", "system.rollout_length=8",
         "system.num_simulations=8", "system.num_minibatches=2",
         "system.epochs=2", "logger.loggers=[]",
         "logger.checkpointing.save_model=false"],
    )
    t0 = time.perf_counter()
    r = run(cfg)
    print(f"AZ identity gate, fused={os.environ.get('STOIX_FUSED_MCTS', '1') != '0'}:"
          f" return {r:.2f} (gate > 8.0, optimum 10.0) in {time.perf_counter() - t0:.1f} s")


if __name__ == "__main__":
    assert torch.cuda.is_available(), "the MCTS probe needs a GPU"
    mode = sys.argv[1] if len(sys.argv) > 1 else "search"
    if mode == "search":
        search_probe()
    elif mode == "sps":
        sps_probe()
    elif mode == "_sps_child":
        sps_child(sys.argv[2], int(sys.argv[3]))
    elif mode == "count":
        count_probe()
    elif mode == "gate":
        gate_probe()
    else:
        raise SystemExit(f"unknown mode {mode!r}")
