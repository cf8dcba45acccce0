"""Sweep wgrad (KPG, NTB) per flagship shape on the GPU and print the
fastest variant for each (bake the winners into wgrad.hip's launcher).
Shapes (S=32768): W2 N=256 K=256; W1 N=256 K=32; Wh N=16 K=256; Wv N=1 K=256.

--pair sweeps the pipelined, paired kernel (ext.wgrad_pair) instead: per
flagship shape its tile / stage-depth variants against the two old launches
it replaces, for layer 1 also the form with the SiLU backward in its staging
(ext.wgrad_pair_act, two stage depths) against silu_bwd + the plain pair, and
the paired reduce against two slab_reduce calls. The
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
        if name != "W1":
            continue
        # layer 1 with the SiLU backward inside the staging (wgrad_pair_act)
        # against silu_bwd + the plain pair; dH and Z stacked [2, S, N] as in
        # the engine, rotating like the sets above
        stk = [(torch.randn(2, S, NS, device=dev, dtype=bf) * 0.1,
                torch.randn(2, S, NS, device=dev, dtype=bf) * 3.0,
                torch.randn(S, K, device=dev, dtype=bf)) for _ in range(nsets // 2 + 1)]
        dZs = torch.zeros(2, S, NS, device=dev, dtype=bf)
        jt = [0]

        def nxt3():
            jt[0] = (jt[0] + 1) % len(stk)
            return stk[jt[0]]

        def unfused():
            dH, Z, X = nxt3()
            ext.silu_bwd(dH, Z, dZs)
            ext.wgrad_pair(dZs[0], X, slabs[0], off, off + NS * K, NS,
                           dZs[1], X, slabs[1], off, off + NS * K, NS)

        def fused(v):
            dH, Z, X = nxt3()
            assert ext.wgrad_pair_act(dH[0], Z[0], X, slabs[0], off, off + NS * K, NS,
                                      dH[1], Z[1], X, slabs[1], off, off + NS * K, NS, v)

        need = 2 * 2 * S * NS * 2 + S * K * 2 + 64 * 4 * 2 * (NS * K + NS)
        print(f"  silu_bwd + pair: {timeit(unfused):.2f} us; fused needs "
              f"{need / 1e6:.1f} MB = {need / 6.3e6:.2f} us at 6.3 TB/s")
        for v, desc in ((0, "2 steps/stage"), (1, "1 step/stage")):
            t = timeit(lambda: fused(v))
            jt[0] = 0
            unfused()
            want = [s.clone() for s in slabs]
            for s in slabs:
                s.fill_(float("nan"))
            jt[0] = 0
            fused(v)
            same = all(torch.equal(a.view(torch.int32)[:, off:off + NS * K + NS],
                                   b.view(torch.int32)[:, off:off + NS * K + NS])
                       for a, b in zip(slabs, want))
            for s in slabs:
                s.zero_()
            print(f"  wgrad_pair_act variant {v} ({desc}): {t:.2f} us, "
                  f"{need / t / 1e6:.2f} TB/s, {'bit-equal' if same else 'MISMATCH'}")
    grads = [torch.zeros(stride, device=dev, dtype=bf) for _ in range(2)]
    e0 = torch.zeros(0, device=dev)
    e1 = torch.zeros(0, dtype=torch.int64, device=dev)
    t2 = timeit(lambda: [ext.slab_reduce(slabs[i], grads[i], e0, e1) for i in range(2)])
    tp = timeit(lambda: ext.slab_reduce_pair(slabs[0], grads[0], e0, e1,
                                             slabs[1], grads[1], e0, e1))
    print(f"reduce: two slab_reduce {t2:.2f} us, slab_reduce_pair {tp:.2f} us")


def main_l2fwd():
    """--l2fwd: the layer-2 forward group at the flagship shape, the fused
    launch (ext.linear_silu_heads_pair) against the two addmm calls and
    silu_heads_fwd it replaces, with and without the value head. Four operand
    sets (about 400 MB) rotate so that the rows come from HBM."""
    import math

    ext = ops.ext(required=True)
    dev, bf, H, NSET = torch.device("cuda:0"), torch.bfloat16, 256, 4
    r = lambda *s: torch.randn(*s, device=dev)
    W2 = (r(2, H, H) / math.sqrt(H)).to(bf)
    b2, Wh, bh = (0.5 * r(2, H)).to(bf), (r(16, H) / math.sqrt(H)).to(bf), r(16).to(bf)
    Wv, bv = (r(H) / math.sqrt(H)).to(bf), r(1).to(bf)
    sets = [dict(H1=r(2, S, H).to(bf), Z2=torch.empty(2, S, H, device=dev, dtype=bf),
                 H2=torch.empty(2, S, H, device=dev, dtype=bf),
                 heads=torch.empty(S, 16, device=dev, dtype=bf),
                 vpred=torch.empty(S, 1, device=dev, dtype=bf)) for _ in range(NSET)]
    none = torch.empty(0, device=dev, dtype=bf)
    it = [0]

    def old(vp):
        b = sets[it[0] % NSET]
        it[0] += 1
        torch.addmm(b2[0], b["H1"][0], W2[0].t(), out=b["Z2"][0])
        torch.addmm(b2[1], b["H1"][1], W2[1].t(), out=b["Z2"][1])
        ext.silu_heads_fwd(b["Z2"], Wh, bh, Wv, bv, b["H2"], b["heads"],
                           b["vpred"] if vp else none)

    def new(vp):
        b = sets[it[0] % NSET]
        it[0] += 1
        assert ext.linear_silu_heads_pair(
            b["H1"], W2[0], b2[0], W2[1], b2[1], Wh, bh, Wv, bv, b["Z2"],
            b["H2"], b["heads"], b["vpred"] if vp else none)

    need = 3 * 2 * S * H * 2 + S * 32  # H1 in, Z2 and H2 out, heads out
    for vp in (False, True):
        t_old, t_new = timeit(lambda: old(vp)), timeit(lambda: new(vp))
        print(f"l2fwd S={S} H={H} vpred={vp}: 2 addmm + silu_heads_fwd "
              f"{t_old:.2f} us; linear_silu_heads_pair {t_new:.2f} us "
              f"({need / t_new / 1e6:.2f} TB/s of the {need / 1e6:.1f} MB needed)")


if __name__ == "__main__":
    if "--l2fwd" in sys.argv[1:]:
        main_l2fwd()
    elif "--pair" in sys.argv[1:]:
        main_pair()
    else:
        main()
