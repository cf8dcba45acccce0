"""GPU tests for ppo_gather_rows (ppo_gather_rows_kernel in
stoix_amd/ops/csrc/mlp.hip): the gather of a whole epoch's rows in one
bandwidth-built launch (STOIX_EPOCH_GATHER). The contract is bit-equality of
every output with ppo_gather / ppo_gather_disc, the one-wave-per-row kernels
it replaces, and that nothing past row n - 1 of any output is touched."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")

ROWS = 5000  # rows of the source arrays
GUARD_ROWS = 5
NAMES = ("obs", "act", "logp", "val", "adv", "tgt")


@pytest.fixture(scope="module")
def ext():
    from stoix_amd import ops

    e = ops.ext(required=True)
    assert e is not None
    return e


@functools.lru_cache(maxsize=None)
def _sources(OBS, ACT, disc):
    """Seeded rollout storage; obs beyond +-10 sigma so the clamp of the
    normalisation is exercised. Never written to."""
    g = torch.Generator().manual_seed(8800 + 11 * OBS + ACT + 100 * disc)
    obs = (torch.randn(ROWS, OBS, generator=g) * 6.0).cuda()
    if disc:
        act = torch.randint(0, 16, (ROWS,), generator=g).cuda()
    else:
        act = torch.randn(ROWS, ACT, generator=g).cuda()
    f = [torch.randn(ROWS, generator=g).cuda() for _ in range(4)]
    mean = torch.randn(OBS, generator=g).cuda()
    var = (torch.rand(OBS, generator=g) * 2.0).cuda()
    var[0] = 0.0  # below the 1e-6 floor
    return obs, act, f, mean, var


@functools.lru_cache(maxsize=None)
def _perm(n):
    """n source rows in random order that contain row 0 and the last row."""
    g = torch.Generator().manual_seed(31 + n)
    p = torch.randperm(ROWS, generator=g)[:n].clone()
    p[n // 2] = ROWS - 1
    p[0 if n == 1 else n - 1] = 0
    if n == 1:
        p[0] = ROWS - 1
    return p.cuda()


def _outputs(n, OBS, ACT, disc):
    """Outputs with GUARD_ROWS sentinel rows after row n - 1."""
    pad = (OBS + 31) // 32 * 32
    m = n + GUARD_ROWS
    o = {"obs": torch.full((m, pad), 7.0, dtype=torch.bfloat16, device="cuda")}
    if disc:
        o["act"] = torch.full((m,), -77, dtype=torch.long, device="cuda")
    else:
        o["act"] = torch.full((m, ACT), 7.0, device="cuda")
    for k in NAMES[2:]:
        o[k] = torch.full((m,), 7.0, device="cuda")
    return o


def _call(fn, idx, src, out, n, norm):
    obs, act, f, mean, var = src
    e = torch.zeros(0, device="cuda")
    return fn(idx, obs, act, f[0], f[1], f[2], f[3],
              *[out[k][:n] for k in NAMES], mean if norm else e, var if norm else e)


def _raw(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else (
        t.view(torch.int32) if t.dtype == torch.float32 else t)


def _check(new, old, n):
    for k in NAMES:
        assert torch.equal(_raw(new[k][:n]), _raw(old[k][:n])), k
        g = new[k][n:]
        assert (g == (-77 if g.dtype == torch.long else 7.0)).all(), f"{k}: guard rows"


@requires_gpu
@pytest.mark.parametrize("n", [1, 67, 384, 4096])
@pytest.mark.parametrize("OBS", [5, 27, 40, 128])
@pytest.mark.parametrize("ACT,disc", [(3, False), (8, False), (1, True)])
@pytest.mark.parametrize("norm", [False, True])
def test_rows_bit_equal_to_one_wave_per_row(ext, n, OBS, ACT, disc, norm):
    src = _sources(OBS, ACT, disc)
    idx = _perm(n)
    assert (idx == 0).any() or n == 1
    assert (idx == ROWS - 1).any()
    old, new = _outputs(n, OBS, ACT, disc), _outputs(n, OBS, ACT, disc)
    _call(ext.ppo_gather_disc if disc else ext.ppo_gather, idx, src, old, n, norm)
    assert _call(ext.ppo_gather_rows, idx, src, new, n, norm) is True
    torch.cuda.synchronize()
    _check(new, old, n)
    # the pad columns are zeros, the valid ones were written
    assert (new["obs"][:n, OBS:].float() == 0).all()
    assert (new["obs"][:n, :OBS] != 7.0).any()


@requires_gpu
@pytest.mark.parametrize("disc", [False, True])
def test_slices_of_one_call_equal_one_call_per_minibatch(ext, disc):
    """Rows [mb * S, (mb + 1) * S) of one n = 4 x 96 call are what the old
    kernel gives for the mb-th index slice."""
    S, n_mb, OBS, ACT = 96, 4, 27, 8
    src = _sources(OBS, ACT, disc)
    idx = _perm(S * n_mb)
    new = _outputs(S * n_mb, OBS, ACT, disc)
    assert _call(ext.ppo_gather_rows, idx, src, new, S * n_mb, True) is True
    for mb in range(n_mb):
        old = _outputs(S, OBS, ACT, disc)
        _call(ext.ppo_gather_disc if disc else ext.ppo_gather,
              idx[mb * S:(mb + 1) * S], src, old, S, True)
        torch.cuda.synchronize()
        for k in NAMES:
            assert torch.equal(_raw(new[k][mb * S:(mb + 1) * S]), _raw(old[k][:S])), (mb, k)


@requires_gpu
def test_shapes_not_taken_launch_nothing(ext):
    """An obs_out width outside {32, 64, 96, 128} and more than 8 continuous
    action columns: False, outputs untouched. Mismatched operands raise."""
    n, OBS = 67, 27
    src = _sources(OBS, 3, False)
    idx = _perm(n)
    out = _outputs(n, OBS, 3, False)
    wide = dict(out, obs=torch.full((n + GUARD_ROWS, 160), 7.0, dtype=torch.bfloat16,
                                    device="cuda"))
    assert _call(ext.ppo_gather_rows, idx, src, wide, n, False) is False
    obs, act, f, mean, var = src
    src9 = (obs, torch.zeros(ROWS, 9, device="cuda"), f, mean, var)
    out9 = dict(out, act=torch.full((n + GUARD_ROWS, 9), 7.0, device="cuda"))
    assert _call(ext.ppo_gather_rows, idx, src9, out9, n, False) is False
    torch.cuda.synchronize()
    for o in (wide, out9):
        for k in NAMES:
            assert (o[k] == 7.0).all(), k
    with pytest.raises(RuntimeError, match="dtype"):
        _call(ext.ppo_gather_rows, idx.int(), src, out, n, False)
    with pytest.raises(RuntimeError, match="shorter than idx"):
        _call(ext.ppo_gather_rows, idx, src, dict(out, adv=out["adv"][:n - 1]), n, False)
