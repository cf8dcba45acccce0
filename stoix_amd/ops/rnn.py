"""Done-masked GRU/LSTM sequence scan with a closed-form backward (K13).

``_RnnScan`` is the recurrent half of ``networks.base.ScannedRNN`` as one
autograd node: it takes the input projections ``xp = x @ W_ih^T + b_ih`` for
all T (hoisted into one GEMM by the caller, whose autograd carries ``dXp`` on
to ``x``, ``W_ih`` and ``b_ih``) and runs the scan over T with the hidden
state reset *before* step t wherever ``resets[t]`` is set.

On the GPU the forward and the backward through time are the two rnn.hip
kernels (``rnn_scan_train_fwd``, bit-equal to the no-grad ``rnn_scan``, and
``rnn_scan_bwd``); the weight and bias gradients are one GEMM and one
reduction over what the backward kernel wrote. On the CPU the same closed
form runs in torch in the input dtype, so fp64 checks the derivation.
"""
from __future__ import annotations

import os

import torch
from torch.autograd.function import once_differentiable

Tensor = torch.Tensor


def rnn_fused_enabled() -> bool:
    """STOIX_FUSED_RNN=0 keeps the training scan on autograd (A/B timing)."""
    return os.environ.get("STOIX_FUSED_RNN", "1") != "0"


def _keep_mask(resets: Tensor, dtype) -> Tensor:
    """[T, B, 1]: 0 where the state is reset before step t, else 1."""
    return (~resets.bool()).to(dtype).unsqueeze(-1)


class _RnnScan(torch.autograd.Function):
    """(xp [T,B,G*H], whh [G*H,H], bhh [G*H], resets [T,B], h0 [B,H],
    c0 [B,H] or None, kind) -> (Hout [T,B,H], hT[, cT]).

    Gate order is r|z|n (GRU) and i|f|g|o (LSTM), as in nn.GRUCell and
    nn.LSTMCell. Saved per step: the activated gates and ``aux`` (GRU: hn =
    h_prev Whn^T + bhn, LSTM: the new cell state); h_prev / c_prev are
    rebuilt from h0 / c0, Hout and aux in the backward.
    """

    @staticmethod
    def forward(ctx, xp, whh, bhh, resets, h0, c0, kind):
        lstm = kind == "lstm"
        T, B, GH = xp.shape
        H = h0.shape[1]
        ctx.lstm = lstm
        ctx.set_materialize_grads(False)
        if xp.is_cuda:
            from stoix_amd.ops import ext

            dev = xp.device
            f32 = dict(dtype=torch.float32, device=dev)
            empty = torch.empty(0, **f32)
            whh16 = whh.detach().to(torch.bfloat16).contiguous()
            rs = resets.to(torch.uint8).contiguous()
            h0c = h0.detach().contiguous()
            c0c = c0.detach().contiguous() if lstm else empty
            Hout = torch.empty(T, B, H, **f32)
            hT = torch.empty(B, H, **f32)
            cT = torch.empty(B, H, **f32) if lstm else empty
            gates = torch.empty(T, B, GH, **f32)
            aux = torch.empty(T, B, H, **f32)
            ext(required=True).rnn_scan_train_fwd(
                xp.detach().contiguous(), whh16, bhh.detach().contiguous(), rs,
                h0c, c0c, Hout, hT, cT, gates, aux, int(lstm),
            )
            # [H, G*H]: the backward's B fragments are then contiguous rows
            w_saved = whh16.t().contiguous()
            ctx.save_for_backward(w_saved, rs, h0c, c0c, Hout, gates, aux)
            return (Hout, hT, cT) if lstm else (Hout, hT)

        keep = _keep_mask(resets, xp.dtype)
        h, c = h0, c0
        outs, gates, aux = [], [], []
        for t in range(T):
            hp = h * keep[t]
            hg = hp @ whh.t() + bhh
            if lstm:
                cp = c * keep[t]
                i, f, g, o = (xp[t] + hg).chunk(4, -1)
                i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
                c = f * cp + i * g
                h = o * torch.tanh(c)
                gates.append(torch.cat([i, f, g, o], -1))
                aux.append(c)
            else:
                xr, xz, xn = xp[t].chunk(3, -1)
                hr, hz, hn = hg.chunk(3, -1)
                r = torch.sigmoid(xr + hr)
                z = torch.sigmoid(xz + hz)
                n = torch.tanh(xn + r * hn)
                h = (1 - z) * n + z * hp
                gates.append(torch.cat([r, z, n], -1))
                aux.append(hn)
            outs.append(h)
        Hout = torch.stack(outs)
        c0s = c0 if lstm else xp.new_empty(0)
        ctx.save_for_backward(whh, resets, h0, c0s, Hout, torch.stack(gates), torch.stack(aux))
        return (Hout, h.clone(), c.clone()) if lstm else (Hout, h.clone())

    @staticmethod
    @once_differentiable
    def backward(ctx, dHout, dhT, dcT=None):
        w_saved, resets, h0, c0, Hout, gates, aux = ctx.saved_tensors
        lstm = ctx.lstm
        T, B, GH = gates.shape
        H = h0.shape[1]
        keep = _keep_mask(resets, Hout.dtype)
        # the gradient of a .sum() arrives as a stride-0 expand
        dHout = torch.zeros_like(Hout) if dHout is None else dHout.to(Hout.dtype).contiguous()
        if Hout.is_cuda:
            from stoix_amd.ops import ext

            empty = torch.empty(0, dtype=torch.float32, device=Hout.device)
            dXp = torch.empty_like(gates)
            dHg = dXp if lstm else torch.empty_like(gates)
            dh0 = torch.empty_like(h0)
            dc0 = torch.empty_like(h0) if lstm else empty
            ext(required=True).rnn_scan_bwd(
                dHout,
                empty if dhT is None else dhT.float().contiguous(),
                empty if dcT is None or not lstm else dcT.float().contiguous(),
                gates, aux, Hout, h0, c0, resets, w_saved,
                dXp, dHg if not lstm else empty, dh0, dc0, int(lstm),
            )
            whh_dtype = torch.float32
        else:
            whh = w_saved
            dh = torch.zeros_like(h0) if dhT is None else dhT.to(h0.dtype)
            dc = torch.zeros_like(h0) if dcT is None or not lstm else dcT.to(h0.dtype)
            dXp_l, dHg_l = [None] * T, [None] * T
            for t in range(T - 1, -1, -1):
                dh = dh + dHout[t]
                if lstm:
                    i, f, g, o = gates[t].chunk(4, -1)
                    c_prev = keep[t] * (c0 if t == 0 else aux[t - 1])
                    tc = torch.tanh(aux[t])
                    dc = dc + dh * o * (1 - tc * tc)
                    d_all = torch.cat(
                        [
                            dc * g * i * (1 - i),
                            dc * c_prev * f * (1 - f),
                            dc * i * (1 - g * g),
                            dh * tc * o * (1 - o),
                        ],
                        -1,
                    )
                    dXp_l[t] = dHg_l[t] = d_all
                    dh = keep[t] * (d_all @ whh)
                    dc = keep[t] * (dc * f)
                else:
                    r, z, n = gates[t].chunk(3, -1)
                    h_prev = keep[t] * (h0 if t == 0 else Hout[t - 1])
                    dn_pre = dh * (1 - z) * (1 - n * n)
                    dz_pre = dh * (h_prev - n) * z * (1 - z)
                    dr_pre = dn_pre * aux[t] * r * (1 - r)
                    dXp_l[t] = torch.cat([dr_pre, dz_pre, dn_pre], -1)
                    dHg_l[t] = torch.cat([dr_pre, dz_pre, dn_pre * r], -1)
                    dh = keep[t] * (dh * z + dHg_l[t] @ whh)
            dXp, dHg = torch.stack(dXp_l), torch.stack(dHg_l)
            dh0, dc0 = dh, dc
            whh_dtype = whh.dtype
        # weight and bias gradients: one GEMM and one reduction over all T
        Hprev = torch.cat([h0.unsqueeze(0), Hout[:-1]], 0) * keep
        dWhh = (dHg.reshape(T * B, GH).t() @ Hprev.reshape(T * B, H)).to(whh_dtype)
        dbhh = dHg.sum((0, 1))
        return dXp, dWhh, dbhh, None, dh0, (dc0 if lstm else None), None


def rnn_scan(xp: Tensor, whh: Tensor, bhh: Tensor, resets: Tensor, h0: Tensor, c0, kind: str):
    """Differentiable done-masked scan; returns (Hout, hT) for ``"gru"`` and
    (Hout, hT, cT) for ``"lstm"``."""
    return _RnnScan.apply(xp, whh, bhh, resets, h0, c0 if kind == "lstm" else None, kind)
