"""The fused deterministic step: the scatter takes the magnitude of d(dnn_input) from the GEMM that wrote it and leaves
its 64-bit row totals to the table optimizer (engine.GatherOp.bwd_calls, optimizer.Optimizer.calls_split) -- against the
same step with MMLREC_DET_FUSED=0 (magnitude pass + finalize launch), bit for bit."""
import pytest

pytestmark = pytest.mark.gpu

# AE-30 is the only workload family whose input gradient the output-stationary GEMM serves (192 <= F * E <= 256, several
# first layers); 0.2 of its vocabularies keeps 2^24 table parameters (the marked streaming update); 16 384 rows is that
# GEMM's smallest batch
WORKLOAD, SCALE, B = "mmoe_ae30", 0.2, 16384


@pytest.fixture()
def env(monkeypatch):
    import torch
    import mmlrec_amd  # noqa: F401
    from mmlrec_amd import _lib as L, workloads as W
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    monkeypatch.delenv("MMLREC_DET_FUSED", raising=False)
    return torch, L, W, monkeypatch


def _runner(torch, W, table_update):
    dev = torch.device("cuda:0")
    model, cfg, vocab, dense = W.build_model(WORKLOAD, dev, vocab_scale=SCALE, seed=0, table_update=table_update)
    g = torch.Generator().manual_seed(3)
    with torch.no_grad():  # (the reference's 1e-4 initialisation gives gradients at Adam's eps)
        for n, p in model.named_parameters():
            if p.dim() == 2:
                scale = 0.05 if n.startswith("embedding") else (2.0 / p.shape[1]) ** 0.5
                p.copy_((torch.randn(p.shape, generator=g) * scale).to(dev))
    model.scatter_mode = "deterministic"
    model.compile("adam", cfg["optim_config"]["loss"], ["auc"])
    model.train()
    runner = model.train_step_runner(B, use_graph=True, split_dense=False)
    return model, cfg, vocab, runner


def _scatter_meta(L, runner):
    lib = L.load()
    calls = [c for part in runner.whole.parts if part[0] == "c" for c in part[1]]
    det = [c for c in calls if c[0] is lib.mml_scatter_bwd_det]
    assert len(det) == 1
    return det[0][-1], calls


def test_fused_step_equals_the_unfused_step_bit_for_bit(env):
    """(e) three steps (eager, capture, replay) from the same seed with the fused launches and with MMLREC_DET_FUSED=0:
    state_dict() bit-equal.  The plan's choice is read from the scatter call's meta, so a silent fall-back fails."""
    torch, L, W, mp = env
    finals = []
    for fused in (True, False):
        if not fused:
            mp.setenv("MMLREC_DET_FUSED", "0")
        model, cfg, vocab, runner = _runner(torch, W, "dense_exact")
        meta, calls = _scatter_meta(L, runner)
        want = (L.SCATTER_DET_AMAX_SUPPLIED | L.SCATTER_DET_DEFER_TOTALS) if fused else 0
        assert meta["det_flags"] == want, meta
        lib = L.load()
        tab_opt = [c for c in calls if c[0] is lib.mml_opt_step_dense and c[-1].get("det_acc64")]
        assert len(tab_opt) == (1 if fused else 0)
        T = W.num_tasks(cfg)
        for i in range(3):
            X, y = W.synth_batch(vocab, 0, B, T, seed=1 + i)
            runner.plan.X.copy_(X.cuda())
            runner.plan.y.copy_(y.cuda())
            runner.run()
        assert runner.whole.n_graphs >= 1
        torch.cuda.synchronize()
        det = runner.plan.ops[0].deterministic
        assert all(int(a.abs().max()) == 0 for a in det["acc64"])       # consumed either way
        finals.append({k: v.detach().clone() for k, v in model.state_dict().items()})
        del model, runner
    assert sum(k.startswith("embedding_dict.") for k in finals[0]) == 30
    for k in finals[0]:
        assert torch.equal(finals[0][k].view(torch.int32), finals[1][k].view(torch.int32)), k


def test_lazy_exact_keeps_the_finalize_launch(env):
    """(f) the row-wise table updates read the fp32 gradient rows: their scatter must not defer the totals."""
    torch, L, W, mp = env
    model, cfg, vocab, runner = _runner(torch, W, "lazy_exact")
    meta, _ = _scatter_meta(L, runner)
    assert not meta["det_flags"] & L.SCATTER_DET_DEFER_TOTALS, meta
