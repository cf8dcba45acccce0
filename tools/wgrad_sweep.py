"""Sweep wgrad (KPG, NTB) per flagship shape on the GPU and print the
fastest variant for each (bake the winners into wgrad.hip's launcher).
Shapes (S=32768): W2 N=256 K=256; W1 N=256 K=32; Wh N=16 K=256; Wv N=1 K=256.

--pair sweeps the pipelined, paired kernel (ext.wgrad_pair) instead: per
flagship shape its tile / stage-depth variants against the two old launches
it replaces, and the paired reduce against two slab_reduce calls. The
operands rotate through more than 256 MB per shape, so the Infinity Cache
does not serve what the engine streams from HBM.
"""
from __future__ import annotations

import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from stoix_amd import ops

S = 32768


def timeit(fn, iters=100, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def main():
    ext = ops.ext(required=True)
    dev = torch.device("cuda:0")
    bf = torch.bfloat16
    shapes = [("W2", 256, 256, 256), ("W1", 256, 32, 256), ("Wh", 16, 256, 16), ("Wv", 1, 256, 16)]
    for name, NV, K, NSTRIDE in shapes:
        dZ = torch.randn(S, NSTRIDE, device=dev, dtype=bf)
        X = torch.randn(S, K, device=dev, dtype=bf)
        # realistic slab: the engine's chain slab has stride ~74.5K floats
        # and this dW sits at a mid-chain offset
        stride = 74512
        off = 8448
        slab = torch.zeros(64, stride, device=dev, dtype=torch.float32)
        NT = (NV + 15) // 16
        results = []
        for kpg in (1, 2, 4, 8):
            if K % (16 * kpg) != 0:
                continue
            for ntb in (1, 4):
                if NT % ntb != 0:
                    continue
                wgs = (NT // ntb) * (K // (16 * kpg)) * 16
                t = timeit(lambda: ext.wgrad(dZ, X, slab, off, off + NV * K, NV, kpg, ntb))
                results.append((t, kpg, ntb, wgs))
        results.sort()
        best = results[0]
        print(f"{name} (N={NV},K={K}): best KPG={best[1]} NTB={best[2]} "
              f"({best[3]} WGs) {best[0]:.2f} us | " +
              " ".join(f"k{k}n{n}={t:.1f}({w}wg)" for t, k, n, w in results))


PAIR_VARIANTS = {
    "W2": ["128n x 256k, 1 step/stage", "64n x 256k, 1 step/stage",
           "128n x 128k, 1 step/stage", "128n x 256k, 2 steps/stage"],
    "W1": ["128n x 32k, 2 steps/stage", "128n x 32k, 1 step/stage",
           "64n x 32k, 2 steps/stage", "128n x 32k, 4 steps/stage"],
    "heads": ["16n x 128k, 2 steps/stage", "16n x 128k, 1 step/stage",
              "16n x 64k, 2 steps/stage", "16n x 128k, 4 steps/stage"],
}


def main_pair():
    ext = ops.ext(required=True)
    dev = torch.device("cuda:0")
    bf = torch.bfloat16
    stride = 74512  # the engine's chain slab stride (floats)
    slabs = [torch.zeros(64, stride, device=dev) for _ in range(2)]
    # name, N_STRIDE, K, (N_VALID actor, critic), dW offset, shared X
    shapes = [("W2", 256, 256, (256, 256), 8448, False),
              ("W1", 256, 32, (256, 256), 0, True),
              ("heads", 16, 256, (16, 1), 70000, False)]
    for name, NS, K, NV, off, shared in shapes:
        per_set = 2 * S * NS * 2 + (1 if shared else 2) * S * K * 2
        nsets = max(2, (300 << 20) // per_set + 1)
        sets = []
        for _ in range(nsets):
            dZ = [torch.randn(S, NS, device=dev, dtype=bf) * 0.1 for _ in range(2)]
            X0 = torch.randn(S, K, device=dev, dtype=bf)
            X = [X0, X0 if shared else torch.randn(S, K, device=dev, dtype=bf)]
            sets.append((dZ, X))
        it = [0]

        def nxt():
            it[0] = (it[0] + 1) % nsets
            return sets[it[0]]

        def old():
            dZ, X = nxt()
            for i in range(2):
                ext.wgrad(dZ[i], X[i], slabs[i], off, off + NV[i] * K, NV[i])

        def pair(v):
            dZ, X = nxt()
            ext.wgrad_pair(dZ[0], X[0], slabs[0], off, off + NV[0] * K, NV[0],
                           dZ[1], X[1], slabs[1], off, off + NV[1] * K, NV[1], v)

        need = per_set + 64 * 4 * (NV[0] * K + NV[0] + NV[1] * K + NV[1])
        t_old = timeit(old)
        print(f"{name}: two old launches {t_old:.2f} us; bytes needed "
              f"{need / 1e6:.1f} MB = {need / 6.3e6:.2f} us at 6.3 TB/s")
        variants = list(enumerate(PAIR_VARIANTS[name]))
        # +4: the same tiles with the slice along blockIdx.x (sharers of a
        # slice's rows on one XCD)
        variants += [(v + 4, d + ", slice-major grid") for v, d in variants[:3:2]]
        for v, desc in variants:
            t = timeit(lambda: pair(v))
            # every variant must give the old kernels' slab bit for bit
            it[0] = 0
            old()
            want = [s.clone() for s in slabs]
            for s in slabs:
                s.fill_(float("nan"))
            it[0] = 0
            pair(v)
            same = all(torch.equal(a.view(torch.int32)[:, off:off + NV[i] * K + NV[i]],
                                   b.view(torch.int32)[:, off:off + NV[i] * K + NV[i]])
                       for i, (a, b) in enumerate(zip(slabs, want)))
            for s in slabs:
                s.zero_()
            print(f"  pair variant {v} ({desc}): {t:.2f} us, "
                  f"{need / t / 1e6:.2f} TB/s, "
                  f"{'bit-equal' if same else 'MISMATCH'}")
    grads = [torch.zeros(stride, device=dev, dtype=bf) for _ in range(2)]
    e0 = torch.zeros(0, device=dev)
    e1 = torch.zeros(0, dtype=torch.int64, device=dev)
    t2 = timeit(lambda: [ext.slab_reduce(slabs[i], grads[i], e0, e1) for i in range(2)])
    tp = timeit(lambda: ext.slab_reduce_pair(slabs[0], grads[0], e0, e1,
                                             slabs[1], grads[1], e0, e1))
    print(f"reduce: two slab_reduce {t2:.2f} us, slab_reduce_pair {tp:.2f} us")


if __name__ == "__main__":
    main_pair() if "--pair" in sys.argv[1:] else main()
