"""Engine-level GPU tests for STOIX_FUSED_DZ1 (layer-1 SiLU backward inside
the wgrad staging) and STOIX_EPOCH_GATHER (one gather per epoch): neither
knob changes a parameter, and the engine picks the per-minibatch gather where
the epoch gather does not apply."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")


def _learner(dz1, eg, num_envs=64, T=8, n_mb=2, norm=False, prefetch="0"):
    """A small fused PPO learner (27 obs / 8 act Ant, H = 256) built with the
    knobs set; they are read in the engine's constructor."""
    from stoix_amd import envs as environments
    from stoix_amd.config import compose
    from stoix_amd.systems.ppo.ff_ppo import PPOLearner
    from stoix_amd.utils.total_timestep_checker import check_total_timesteps

    cfg = compose(
        "default/anakin/default_ff_ppo_continuous.yaml",
        ["env=brax/ant", f"arch.total_num_envs={num_envs}",
         "arch.total_timesteps=null", "arch.num_updates=4",
         "arch.num_evaluation=1", "arch.seed=11",
         f"system.rollout_length={T}", f"system.num_minibatches={n_mb}",
         "system.epochs=1", "logger.loggers=[]", "system.compute_dtype=bf16",
         f"system.normalize_observations={'true' if norm else 'false'}"],
    )
    cfg.arch.n_devices = 1
    check_total_timesteps(cfg)
    device = torch.device("cuda:0")
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("STOIX_FUSED_DZ1", dz1)
        mp.setenv("STOIX_EPOCH_GATHER", eg)
        mp.setenv("STOIX_FUSED_PREFETCH", prefetch)
        mp.setenv("STOIX_FUSED_STRICT", "1")
        torch.manual_seed(11)
        env = environments.make_single(cfg, num_envs, device, seed=3)
        learner = PPOLearner(cfg, env, device)
    F_ = learner.fused
    assert F_ is not None
    assert F_.norm == norm
    assert F_.fused_dz1 == (dz1 != "0")
    return learner


def _params_after_one_step(norm):
    snaps = {}
    for dz1, eg in itertools.product("01", "01"):
        learner = _learner(dz1, eg, norm=norm)
        assert learner.fused.epoch_gather == (eg != "0")
        learner.update_step()
        torch.cuda.synchronize()
        snaps[(dz1, eg)] = learner.snapshot_params()
        del learner
    base = snaps[("0", "0")]
    n = 0
    for key, snap in snaps.items():
        for net in ("actor", "critic"):
            for name, want in base[net].items():
                assert torch.isfinite(want).all()
                assert torch.equal(snap[net][name], want), f"{key}: {net}.{name}"
                n += 1
    assert n >= 4 * 10


@requires_gpu
def test_knobs_do_not_change_an_update_step():
    """64 envs, T = 8, 2 minibatches: after one update_step from the same
    seed every parameter is equal across the four knob combinations."""
    _params_after_one_step(norm=False)


@requires_gpu
def test_knobs_do_not_change_an_update_step_with_obs_normalisation():
    """The same with observation normalisation on: the epoch gather reads the
    gmean/gvar snapshot the per-minibatch gathers read."""
    _params_after_one_step(norm=True)


@requires_gpu
def test_epoch_gather_fills_what_the_minibatch_gathers_fill():
    """After an update step the epoch buffers hold, slice by slice, the rows
    the per-minibatch gather leaves in its workspace for the last minibatch,
    and the dZ1 buffer of the fused engine was never written."""
    on, off = _learner("1", "1"), _learner("0", "0")
    for L in (on, off):
        L.update_step()
    torch.cuda.synchronize()
    Fon, Foff = on.fused, off.fused
    S, last = Fon.S, int(on.sys.num_minibatches) - 1
    assert torch.equal(on.perm_buf, off.perm_buf)
    w = Fon.ws_mb[last]
    assert w.Xmb.data_ptr() == Fon.ws_epoch.Xmb[last * S:].data_ptr()
    assert w.Xmb.data_ptr() % 16 == 0 and w.act.data_ptr() % 16 == 0
    for a, b in ((w.Xmb, Foff.Xmb), (w.act, Foff.act_mb), (w.logp, Foff.logp_mb),
                 (w.val, Foff.val_mb), (w.adv, Foff.adv_mb), (w.tgt, Foff.tgt_mb)):
        assert torch.equal(a, b)
    assert (Fon.dZ1 == 0).all() and (Foff.dZ1 != 0).any()


@requires_gpu
def test_engine_stays_on_the_minibatch_gather_where_the_epoch_one_does_not_apply():
    """65 envs, T = 8, 8 minibatches give S = 65 rows, S % 4 != 0: the slice
    bases would not be 16-byte aligned, so the engine allocates no epoch
    buffers and keeps ppo_gather per minibatch whatever the knob says; so does
    the prefetch knob. (No update step here: the layer-1 and wgrad kernels
    take S % 128 == 0 only, with either gather, so an engine with such an S
    cannot run a minibatch. With T = 8 and 2 minibatches, 65 envs give
    S = 260, a multiple of 4, which is on the epoch gather.)"""
    odd = _learner("1", "1", num_envs=65, n_mb=8)
    assert odd.fused.S == 65
    assert odd.fused.epoch_gather is False and not hasattr(odd.fused, "ws_epoch")
    aligned = _learner("1", "1", num_envs=65, n_mb=2)
    assert aligned.fused.S == 260 and aligned.fused.epoch_gather is True
    pre = _learner("1", "1", prefetch="1")
    assert pre.fused.prefetch and pre.fused.epoch_gather is False
