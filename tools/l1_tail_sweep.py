"""Time the paired layer-1 forward and the two-launch optimiser tail against
the launches they replace, at the flagship shapes (S = 32768, H = 256,
K1P = 32/64/96; chains of 78352 and 74497 elements).

The outputs (layer 1) and the slabs (tail) rotate through more than 256 MB,
so the Infinity Cache does not absorb what the engine streams to and from
HBM. Times are host-side averages over back-to-back launches.
"""
from __future__ import annotations

import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from stoix_amd import ops

S, H = 32768, 256


def timeit(fn, iters=200, warmup=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def layer1(ext, dev):
    bf = torch.bfloat16
    for K in (32, 64, 96):
        X = torch.randn(S, K, device=dev, dtype=bf)
        W = [torch.randn(H, K, device=dev, dtype=bf) * 0.3 for _ in range(2)]
        b = [torch.randn(H, device=dev) for _ in range(2)]
        per_set = 4 * S * H * 2
        nsets = (300 << 20) // per_set + 1
        sets = [(torch.empty(2, S, H, device=dev, dtype=bf),
                 torch.empty(2, S, H, device=dev, dtype=bf)) for _ in range(nsets)]
        it = [0]

        def nxt():
            it[0] = (it[0] + 1) % nsets
            return sets[it[0]]

        def old():
            Z, Hh = nxt()
            ext.linear_silu(X, W[0], b[0], Z[0], Hh[0], 1)
            ext.linear_silu(X, W[1], b[1], Z[1], Hh[1], 1)

        def new():
            Z, Hh = nxt()
            ext.linear_silu_pair(X, W[0], b[0], Z[0], Hh[0], W[1], b[1], Z[1], Hh[1])

        t_old, t_new = timeit(old), timeit(new)
        mb = per_set / 1e6
        print(f"layer 1 K={K}: 2 x linear_silu {t_old:6.2f} us ({mb / t_old:.2f} TB/s), "
              f"linear_silu_pair {t_new:6.2f} us ({mb / t_new:.2f} TB/s)")


def tail(ext, dev):
    ns = (78352, 74497)
    nsets = (300 << 20) // (64 * 4 * sum(ns)) + 1
    slabs = [[torch.randn(64, n, device=dev) for n in ns] for _ in range(nsets)]
    g16 = [torch.zeros(n, device=dev, dtype=torch.bfloat16) for n in ns]
    p = [torch.randn(n, device=dev) for n in ns]
    m = [torch.zeros(n, device=dev) for n in ns]
    v = [torch.zeros(n, device=dev) for n in ns]
    p16 = [torch.zeros(n, device=dev, dtype=torch.bfloat16) for n in ns]
    sq = [torch.zeros(1 + 2048, device=dev) for _ in ns]
    st = [torch.zeros(1, device=dev, dtype=torch.int64) for _ in ns]
    cnt = [torch.zeros(1, device=dev, dtype=torch.int32) for _ in ns]
    hyper = (0.9, 0.999, 1e-5, 0.5)
    it = [0]

    def nxt():
        it[0] = (it[0] + 1) % nsets
        return slabs[it[0]]

    def red_old():
        s = nxt()
        ext.slab_reduce_pair(s[0], g16[0], sq[0], st[0], s[1], g16[1], sq[1], st[1])

    def red_new():
        s = nxt()
        ext.slab_reduce_norm_pair(s[0], g16[0], sq[0], st[0], cnt[0],
                                  s[1], g16[1], sq[1], st[1], cnt[1])

    def adam_old():
        for i in range(2):
            ext.fused_adam_bf16(p[i], g16[i], m[i], v[i], sq[i], st[i], p16[i], 3e-4,
                                *hyper, 1.0, 0)

    def adam_new():
        ext.adam_pair(p[0], g16[0], m[0], v[0], sq[0], st[0], p16[0], 3e-4,
                      p[1], g16[1], m[1], v[1], sq[1], st[1], p16[1], 3e-4, *hyper, 1.0)

    def tail_old():
        red_old()
        adam_old()

    def tail_new():
        red_new()
        adam_new()

    mb = 64 * 4 * sum(ns) / 1e6
    t = {f.__name__: timeit(f) for f in (red_old, red_new, adam_old, adam_new,
                                         tail_old, tail_new)}
    print(f"slab_reduce_pair {t['red_old']:6.2f} us ({mb / t['red_old']:.2f} TB/s), "
          f"slab_reduce_norm_pair {t['red_new']:6.2f} us ({mb / t['red_new']:.2f} TB/s)")
    print(f"2 x fused_adam_bf16 (4 launches) {t['adam_old']:6.2f} us, "
          f"adam_pair {t['adam_new']:6.2f} us")
    print(f"tail: five launches {t['tail_old']:6.2f} us, two launches {t['tail_new']:6.2f} us")


def main():
    ext = ops.ext(required=True)
    dev = torch.device("cuda:0")
    layer1(ext, dev)
    tail(ext, dev)


if __name__ == "__main__":
    main()
