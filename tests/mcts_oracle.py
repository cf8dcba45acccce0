"""A deterministic model and a scalar oracle shared by the MCTS step tests
(not a test file).

``make_recurrent_fn`` is a ``recurrent_fn`` made of integer hash arithmetic in
torch, so it gives the same rows on every device and both search paths see
identical inputs. ``oracle_search`` is the search written per tree in plain
Python over numpy float32 scalars, from the description of the two steps
(ops/csrc/mcts.hip's header), not from the batched torch code: every
operation is one correctly rounded f32 operation, so the batched paths must
match it bit for bit.
"""
import numpy as np
import torch

from stoix_amd.search import mcts

_M31 = 0x7FFFFFFF
# few distinct logits, so that equal priors (arg-max ties) are common
_LOGITS = (-1.0, 0.0, 0.0, 0.5, 2.0)
C_PUCT = 1.25


def _mix(h, a):
    """New 31-bit hash of (h, action); int64 arithmetic that never overflows."""
    x = (h * 1103515245 + (a + 1) * 40503 + 12345) & _M31
    x = ((x ^ (x >> 15)) * 2246822519) & _M31
    return x ^ (x >> 13)


_TABLES = {}


def _logit_table(device):
    """The logit table on ``device``, copied there once: a host-to-device copy
    per call would put a synchronisation into every simulation."""
    if device not in _TABLES:
        _TABLES[device] = torch.tensor(_LOGITS, device=device)
    return _TABLES[device]


def _rows(x, A, mode):
    """(reward [B], discount [B], logits [B, A], value [B]) of hash x [B]."""
    f = torch.float32
    table = _logit_table(x.device)
    arange = torch.arange(A, device=x.device)
    logits = table[((x.unsqueeze(1) >> 12) * 31 + arange * 17) % len(_LOGITS)]
    if mode == "flat":  # min_q == max_q: the span clamp is active, scores tie
        zero = torch.zeros(x.shape, dtype=f, device=x.device)
        discount = torch.where(((x >> 4) & 7) == 0, 0.0, 0.97).to(f)
        return zero, discount, logits, zero.clone()
    reward = ((x & 15) - 8).to(f) / 16
    discount = torch.where(((x >> 4) & 7) == 0, 0.0, 0.97).to(f)  # 1/8 terminal
    value = (((x >> 7) & 31) - 16).to(f) / 32
    return reward, discount, logits, value


def make_recurrent_fn(A, mode):
    """``recurrent_fn`` over the embedding {"h": int64 [B, 1]}.

    "bushy": hashed rewards, values and priors, an eighth of the nodes
    terminal. "chain": action 0 has a dominant prior and the only positive
    reward, so every simulation extends one path and the tree reaches depth
    S - 1, the longest walk. "flat": all rewards and values zero.
    """
    assert mode in ("bushy", "chain", "flat")

    def fn(embedding, action):
        x = _mix(embedding["h"].squeeze(1), action)
        reward, discount, logits, value = _rows(x, A, mode)
        if mode == "chain":
            reward = torch.where(action == 0, 0.5, -0.5).to(torch.float32)
            discount = torch.full_like(reward, 0.97)
            value = torch.full_like(reward, 0.25)
            logits = logits.clone()
            logits[:, 0] = 8.0
        return {"h": x.unsqueeze(1)}, reward, discount, logits, value

    return fn


def make_root(B, A, mode, device="cpu"):
    """(root_embedding, root_prior [B, A], root_value [B])."""
    h = torch.arange(B, dtype=torch.long, device=device) * 7919 + 17
    _, _, logits, value = _rows(_mix(h, torch.zeros_like(h)), A, mode)
    if mode == "chain":
        logits = logits.clone()
        logits[:, 0] = 8.0
    return {"h": h.unsqueeze(1)}, torch.softmax(logits, dim=-1), value


def new_search(B, A, S, mode, device="cpu"):
    """(arena, emb_arena, recurrent_fn) with the root in place, S slots to grow."""
    emb, prior, value = make_root(B, A, mode, device)
    arena, emb_arena = mcts._new_search(emb, prior, value, S)
    return arena, emb_arena, make_recurrent_fn(A, mode)


ARENA_FIELDS = (
    "visit", "value_sum", "reward", "discount", "prior", "children", "parent",
    "act_from_parent", "min_q", "max_q",
)


def arena_tensors(arena):
    return {k: getattr(arena, k) for k in ARENA_FIELDS}


def clone_arena(arena):
    out = mcts._Arena(1, 1, 1, arena.visit.device, None)
    for k in ARENA_FIELDS + ("batch",):
        setattr(out, k, getattr(arena, k).clone())
    return out


def assert_arenas_equal(got, want, what=""):
    for k in ARENA_FIELDS:
        a, b = getattr(got, k), getattr(want, k)
        assert a.dtype == b.dtype and torch.equal(a, b), f"{what}: arena.{k} differs"


# ------------------------------------------------------------ scalar oracle

_F = np.float32


class _Tree:
    """One tree of N slots over numpy float32 scalars."""

    def __init__(self, N, A, prior0, value0):
        self.N, self.A = N, A
        self.visit = [_F(0)] * N
        self.value_sum = [_F(0)] * N
        self.reward = [_F(0)] * N
        self.discount = [_F(0)] * N
        self.prior = [[_F(0)] * A for _ in range(N)]
        self.children = [[-1] * A for _ in range(N)]
        self.parent = [-1] * N
        self.act_from_parent = [0] * N
        self.prior[0] = [_F(p) for p in prior0]
        self.discount[0] = _F(1)
        self.visit[0] = _F(1)
        self.value_sum[0] = _F(value0)
        self.min_q = min(_F(1e9), _F(value0))
        self.max_q = max(_F(-1e9), _F(value0))

    def select(self, c_puct):
        cp = _F(c_puct)
        one, zero = _F(1), _F(0)
        span = max(self.max_q - self.min_q, _F(1e-3))
        node = 0
        for _ in range(self.N):
            pv = self.visit[node]
            pq = self.value_sum[node] / max(pv, one) if pv > 0 else zero
            parent_qn = (pq - self.min_q) / span
            root_n = np.sqrt(max(pv, one))
            best, best_a = None, -1
            for a in range(self.A):
                c = self.children[node][a]
                if c >= 0:
                    cv = self.visit[c]
                    q = self.value_sum[c] / max(cv, one)
                    q_edge = self.reward[c] + self.discount[c] * q
                else:
                    cv, q_edge = zero, zero
                qn = (q_edge - self.min_q) / span if cv > 0 else parent_qn
                score = qn + ((cp * self.prior[node][a]) * root_n) / (one + cv)
                assert score.dtype == np.float32
                if best is None or score > best:  # ties keep the lowest action
                    best, best_a = score, a
            if self.children[node][best_a] < 0:
                return node, best_a
            node = self.children[node][best_a]
        raise AssertionError("a path longer than the tree")

    def expand_backup(self, new, sp, sa, reward, discount, prior, value):
        self.reward[new], self.discount[new] = _F(reward), _F(discount)
        self.prior[new] = [_F(p) for p in prior]
        self.parent[new], self.act_from_parent[new] = sp, sa
        self.children[sp][sa] = new
        g, cur = _F(value), new
        while cur >= 0:
            self.visit[cur] = self.visit[cur] + _F(1)
            self.value_sum[cur] = self.value_sum[cur] + g
            q = self.value_sum[cur] / max(self.visit[cur], _F(1))
            self.min_q, self.max_q = min(self.min_q, q), max(self.max_q, q)
            g = self.reward[cur] + self.discount[cur] * g
            cur = self.parent[cur]


def oracle_search(B, A, S, mode, c_puct=C_PUCT):
    """The finished arena fields of S simulations as CPU tensors, keyed like
    ARENA_FIELDS, and the node depths [B, S + 1]. Each simulation's rows come
    from the same ``recurrent_fn``, asked at the oracle's own selections."""
    emb, prior0, value0 = make_root(B, A, mode)
    fn = make_recurrent_fn(A, mode)
    N = S + 1
    trees = [_Tree(N, A, prior0[b].numpy(), value0[b].numpy()) for b in range(B)]
    h = torch.zeros(B, N, dtype=torch.long)
    h[:, 0] = emb["h"].squeeze(1)
    rows = torch.arange(B)
    for sim in range(1, N):
        sel = [t.select(c_puct) for t in trees]
        sp = torch.tensor([s[0] for s in sel])
        sa = torch.tensor([s[1] for s in sel])
        new_emb, reward, discount, logits, value = fn({"h": h[rows, sp].unsqueeze(1)}, sa)
        h[:, sim] = new_emb["h"].squeeze(1)
        prior = torch.softmax(logits, dim=-1).numpy()
        for b, t in enumerate(trees):
            t.expand_backup(sim, sel[b][0], sel[b][1], reward[b].numpy(),
                            discount[b].numpy(), prior[b], value[b].numpy())
    f = lambda name, dtype: torch.tensor(
        np.array([getattr(t, name) for t in trees]), dtype=dtype)
    out = {k: f(k, torch.float32) for k in
           ("visit", "value_sum", "reward", "discount", "prior", "min_q", "max_q")}
    out.update({k: f(k, torch.long) for k in ("children", "parent", "act_from_parent")})
    depth = torch.zeros(B, N, dtype=torch.long)
    for s in range(1, N):
        depth[:, s] = depth[rows, out["parent"][:, s]] + 1
    return out, depth
