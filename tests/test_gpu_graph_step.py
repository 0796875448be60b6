"""Captured, replayed training steps (driver.make_step(launch="graph")) against the eager step for STiL and every baseline:
the same losses, parameters, Adam state, queues, ring pointers, logged values and train metrics, bit for bit, with rings that
wrap and an epoch boundary that re-captures the step.  Also: the deferred gradient reductions with a duplicate destination at
a low arena offset, and re-captures that do not pile up memory."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FL = [3, 4] + [1] * 3
K = 5
B = 16
STEPS = 8


def _dev(obj):
    if torch.is_tensor(obj):
        return obj.cuda()
    if isinstance(obj, dict):
        return {k: _dev(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_dev(v) for v in obj)
    return obj


def _stil_hp(**over):
    hp = dict(model="resnet18", embedding_dim=512, img_size=64, field_lengths=FL, num_classes=K, start_epoch=1, batch_size=B, th1=0.3)
    hp.update(over)
    return hp


def _match_hp(**over):
    from oracle import match_oracle as XO
    hp = XO.default_hparams(model="resnet18", embedding_dim=512, img_size=64, field_lengths=FL, num_classes=K, batch_size=B, start_epoch=1,
                            co_threshold=0.3, contrast_th=0.3, sim_threshold=0.3, **over)
    return dict(vars(hp))


def _stil_batches():
    from stil_tta_amd.driver import synthetic_batch
    return [synthetic_batch(FL, K, B, 64, seed=100 + s, device="cuda") for s in range(STEPS)]


def _match_batches(views):
    from oracle import match_oracle as XO
    from types import SimpleNamespace
    hp = SimpleNamespace(**_match_hp())
    out = []
    for s in range(STEPS):
        b = XO.synthetic_batch(hp, B, seed=200 + s, views=views)
        out.append(_dev(b))
    return out


def _proto(m):
    m.prototypes.copy_(torch.nn.functional.normalize(torch.randn(K, 128, generator=torch.Generator().manual_seed(1))).cuda())


def _case(algo):
    """-> (make model, batches, preset(model)): rings and queues placed so that each of them wraps within the 8 steps"""
    from stil_tta_amd import STiLModel
    from stil_tta_amd.match import CoMatch, FreeMatch, SimMatch
    from stil_tta_amd.mmatch import CoTraining, MMatch
    import stil_tta_amd.mmatch as MM

    def da_near_end(m):
        m.DA_ptr.fill_(m.DA_len - 3)
    if algo == "stil":
        return (lambda: STiLModel(_stil_hp())), _stil_batches(), _proto
    if algo == "stil_DA":
        return (lambda: STiLModel(_stil_hp(DA=True))), _stil_batches(), lambda m: (_proto(m), da_near_end(m))
    if algo == "stil_saint":
        return (lambda: STiLModel(_stil_hp(tabular_encoder="saint"))), _stil_batches(), _proto
    if algo == "mmatch":
        def pre(m):
            m.embed_queue_ptr.fill_(MM.BANK - 40)      # 16 rows per step: truncated at the end after three steps, then from 0
            da_near_end(m)
        return (lambda: MMatch(_stil_hp(DA=True))), _stil_batches(), pre
    if algo == "cotraining":
        return (lambda: CoTraining(_stil_hp())), _stil_batches(), lambda m: None
    if algo == "comatch":
        def pre(m):
            m.model.hist_prob = [torch.softmax(torch.randn(K, generator=torch.Generator().manual_seed(i)), 0).cuda() for i in range(125)]
        return (lambda: CoMatch(_match_hp(K=40))), _match_batches(3), pre   # queues of 40 slots, 14 / 16 rows per step
    if algo == "simmatch":
        return (lambda: SimMatch(_match_hp(K=64))), _match_batches(2), lambda m: da_near_end(m)
    if algo == "freematch":
        return (lambda: FreeMatch(_match_hp())), _match_batches(2), lambda m: None
    raise KeyError(algo)


def _train(algo, launch):
    from stil_tta_amd.driver import make_step, train_step
    from stil_tta_amd.flat import StilAdam
    make, batches, pre = _case(algo)
    torch.manual_seed(0)
    m = make()
    m.setup_device("cuda")
    m.train()
    pre(m)
    opt = StilAdam(m.flat, lr=1e-3)
    if launch == "graph":
        m.reserve_train_metrics(STEPS * B)
        step = make_step(m, opt, batches[0], launch="graph")
        assert step.launch == "graph"
    else:
        step = lambda b: train_step(m, opt, b)  # noqa: E731
    losses = []
    for i, b in enumerate(batches):
        m.current_epoch = 0 if i < STEPS // 2 else 2      # crosses start_epoch = 1 halfway: the loss changes, the step re-captures
        losses.append(step(b).clone())
    torch.cuda.synchronize()
    if launch == "graph":
        assert step.captures == 2 and step.eager_steps == 0
    return m, losses


@pytest.mark.parametrize("algo", ["stil", "stil_DA", "stil_saint", "mmatch", "comatch", "simmatch", "freematch", "cotraining"])
def test_replay_equals_eager(algo):
    me, le = _train(algo, "eager")
    mg, lg = _train(algo, "graph")
    for i, (a, b) in enumerate(zip(le, lg)):
        assert torch.equal(a, b), (i, float(a), float(b))
    sde, sdg = me.state_dict(), mg.state_dict()
    assert list(sde) == list(sdg)
    for k in sde:
        assert torch.equal(sde[k], sdg[k]), k
    for name in ("params", "ema", "exp_avg", "exp_avg_sq", "steps"):
        assert torch.equal(getattr(me.flat, name), getattr(mg.flat, name)), name
    for (n, a), (_, b) in zip(me.named_buffers(), mg.named_buffers()):   # non-persistent queues and ring pointers included
        assert torch.equal(a, b), n
    assert set(me.logged) == set(mg.logged)
    for k in me.logged:
        assert torch.equal(torch.as_tensor(me.logged[k]), torch.as_tensor(mg.logged[k])), k
    for name in ("acc_train", "auc_train", "acc_train_unlabelled", "auc_train_unlabelled"):
        a, b = getattr(me, name).compute(), getattr(mg, name).compute()
        assert torch.equal(a, b), (name, float(a), float(b))
    assert mg.auc_train.reserved and not me.auc_train.reserved


def test_ring_pointers_wrap():
    """The device-side ring pointers of the cases above really wrap (eager run: the reference's arithmetic)."""
    m, _ = _train("mmatch", "eager")
    import stil_tta_amd.mmatch as MM
    p = MM.BANK - 40
    for _ in range(STEPS):
        p = (p + min(B, MM.BANK - p)) % MM.BANK
    assert int(m.embed_queue_ptr) == p and int(m.DA_ptr) == (m.DA_len - 3 + STEPS) % m.DA_len
    c, _ = _train("comatch", "eager")
    assert int(c.model._hist_n) == 128 and int(c.model._hist_pos) == (125 + STEPS) % 128
    ps = 0
    for _ in range(STEPS):
        ps = (ps + min(14, 40 - ps)) % 40
    assert int(c.model.queue_ptr_s) == ps


def test_deferred_reduce_duplicate_slot_at_low_offset(monkeypatch):
    """ops._DeferredReduce: a second contribution to one gradient slot flushes the pending jobs -- but the second job's partials
    still sit in the arena, at a low offset.  Larger products deferred after it must not be handed that region."""
    from stil_tta_amd import ops
    monkeypatch.setattr(ops._defer, "mode", "auto")
    g = torch.Generator().manual_seed(11)
    small = [(torch.randn(512, 32, generator=g).cuda(), torch.randn(512, 64, generator=g).cuda()) for _ in range(2)]
    big = [(torch.randn(4096, 256, generator=g).cuda(), torch.randn(4096, 512, generator=g).cuda()) for _ in range(3)]

    def run():
        w = torch.full((32, 64), 0.5, device="cuda")
        outs = [torch.zeros(256, 512, device="cuda") for _ in big]
        for dy, x in small:                 # job A at offset 0, job B (same slot) right above it: B's add flushes A
            ops.wgrad_tn(dy, x, w, 512, 32, 64, accumulate=1, slot=True)
        for (dy, x), o in zip(big, outs):   # larger allocations while B is pending
            ops.wgrad_tn(dy, x, o, 4096, 256, 512, accumulate=1, slot=True)
        ops.join_side()
        torch.cuda.synchronize()
        return [w] + outs

    ref = run()
    with ops.deferring():
        for d in list(ops._defer.st.values()):
            d["off"], d["jobs"], d["dsts"] = 0, [], set()
        got = run()
    for a, b in zip(ref, got):
        assert torch.equal(a, b)


def test_recapture_does_not_grow_memory():
    """Five re-captures (a new learning rate each) release the previous graph and reuse one warm-up stream's arena."""
    from stil_tta_amd import STiLModel, ops
    from stil_tta_amd.driver import make_step
    from stil_tta_amd.flat import StilAdam
    torch.manual_seed(0)
    m = STiLModel(_stil_hp(start_epoch=0))
    m.setup_device("cuda"); m.train(); m.current_epoch = 1
    _proto(m)
    opt = StilAdam(m.flat, lr=1e-3)
    b = _stil_batches()[0]
    step = make_step(m, opt, b, launch="graph")
    step(b)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    for i in range(5):
        opt.param_groups[0]["lr"] = 1e-3 * (0.5 ** (i + 1))
        step(b)
        torch.cuda.synchronize()
    assert step.captures == 6
    arena = max(d["size"] for d in ops._defer.st.values())
    grown = torch.cuda.memory_allocated() - base
    assert grown <= arena, f"{grown / 2**20:.1f} MiB more after five re-captures (one arena: {arena / 2**20:.0f} MiB)"
