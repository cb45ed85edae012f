"""A training run that can be stopped and continued: the optimizer's state in and out of the library (svg_transformer_set_tensor,
svg_transformer_optim_step_count / _set_optim_step_count), the averaged weights the update kernel keeps (svg_transformer_ema_configure,
SVG_TENSOR_EMA) and the trainer's --save_state / --old_state / --lr_schedule / --ema_decay around them.

Models and batches are those of tests/test_train_optim_gpu.py: KW (dim_model 176) has tensors on both sides of the optimizer's
65 536-element chunk boundary, TINY (dim_model 32) serves everything else; batches of 2-3 rows and 7 tokens."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sd_video_gen_amd import _lib  # noqa: E402
from sd_video_gen_amd import config as svg_config  # noqa: E402
from test_train_gpu import cfg_of  # noqa: E402
from test_train_optim_gpu import F, FEAT, KW, MIX, TINY, batch, make_model, names_of, same_bits, state_of, wide_sd  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")
U = 2.0 ** -24          # relative error bound of one f32 rounding
DENORM = 2.0 ** -149    # absolute error floor of an f32 result (the smallest subnormal)
DECAY = 0.9


def tiny_sd():
    return torch.load(os.path.join(GOLD, "transformer_tiny.pt"))["state_dict"]


def ema_of(m):
    prm = dict(m.named_parameters())
    return {k: m._ctx.transformer_tensor(k, prm[k], _lib.SVG_TENSOR_EMA) for k in names_of(m)}


def full_state(m):
    """everything the next step depends on, read from the library: (p, exp_avg, exp_avg_sq) per tensor, the averaged weights, the step count"""
    return state_of(m), ema_of(m), m._ctx.transformer_optim_step_count()


def same_full(a, b):
    return same_bits(a[0], b[0]) and same_bits(a[1], b[1]) and a[2] == b[2]


# ---- 1. round trip ------------------------------------------------------------------------------------------------------------
def test_state_round_trip_through_a_fresh_context(ctx):
    sd = wide_sd()
    m = make_model("model_10_26", ctx, sd, **KW)
    m.train()
    m.ema_configure(DECAY)
    for i in range(3):
        m.training_loss(cfg_of(F, FEAT, MIX, seed=i), batch(2, 30 + i).cuda(), backward=1)
        m.adam_step(1e-3)
    state = m.optimizer_state()
    assert state["step"] == 3 and state["ema"] is not None
    assert set(state["exp_avg"]) == set(state["exp_avg_sq"]) == set(state["ema"]) == set(names_of(m))
    assert all(not t.is_cuda for part in ("exp_avg", "exp_avg_sq", "ema") for t in state[part].values())
    weights = {k: v.cpu().clone() for k, v in m.state_dict().items()}
    assert any(float(state["exp_avg"][k].abs().max()) > 0 for k in state["exp_avg"])
    assert not same_bits(state["ema"], {k: weights[k] for k in state["ema"]})              # three steps behind the weights

    other = make_model("model_10_26", _lib.Context(0), weights, **KW)
    other.load_optimizer_state(state)
    back = other.optimizer_state()
    assert back["step"] == 3
    for part in ("exp_avg", "exp_avg_sq", "ema"):
        assert same_bits(back[part], state[part]), part
    # the state the restore created is the state right after creation: no gradients to step on
    with pytest.raises(ValueError, match="no gradients yet"):
        other.optim_step(1e-3)
    assert all(float(other.grad_of(k).abs().max()) == 0.0 for k in names_of(other)[:4])


# ---- 2. exact resume -----------------------------------------------------------------------------------------------------------
def test_resume_is_exact_and_a_weights_only_resume_is_not():
    sd, p, lr, wd = tiny_sd(), 0.1, 2e-3, 0.01
    pairs = [(batch(2, 200 + 2 * i).cuda(), batch(3, 201 + 2 * i).cuda()) for i in range(4)]
    seed0 = 5000
    box = {}

    def fresh(weights):
        m = make_model("model_10_26", _lib.Context(0), weights, dropout_p=p, **TINY)
        m.train()
        return m

    def steps(m, lo, hi):
        for i in range(lo, hi):
            for j, nb in enumerate(pairs[i]):                       # the trainer's sequence: one more per micro-batch
                m.training_loss(cfg_of(F, FEAT, MIX, dropout_p=p, seed=seed0 + 2 * i + j + 1), nb, backward=1 if j == 0 else _lib.SVG_BACKWARD_ACCUMULATE)
            if "max_norm" not in box:
                box["max_norm"] = 0.25 * 0.5 * m.grad_norm()        # a quarter of the first step's norm: clipping acts at every step
            norm = m.optim_step(lr, weight_decay=wd, decoupled=True, max_grad_norm=box["max_norm"], grad_scale=0.5, read_norm=True)
            assert box["max_norm"] / (norm + 1e-6) < 1.0, i

    whole = fresh(sd)
    whole.ema_configure(DECAY)
    steps(whole, 0, 4)
    want = full_state(whole)
    assert want[2] == 4

    first = fresh(sd)
    first.ema_configure(DECAY)
    steps(first, 0, 2)
    saved_opt = first.optimizer_state()
    saved_w = {k: v.cpu().clone() for k, v in first.state_dict().items()}
    del first

    second = fresh(sd)
    second.load_state_dict(saved_w)
    second.load_optimizer_state(saved_opt)
    second.ema_configure(DECAY)
    steps(second, 2, 4)
    assert same_full(full_state(second), want)

    # what --resume alone does: the weights, and Adam starts again (the comparison above can fail)
    cold = fresh(sd)
    cold.load_state_dict(saved_w)
    cold.ema_configure(DECAY)
    steps(cold, 2, 4)
    got = full_state(cold)
    assert got[2] == 2
    assert not same_bits(got[0], want[0]) and not same_bits(got[1], want[1])


# ---- 3. the averaged weights against their stated expression -----------------------------------------------------------------------
def test_ema_against_its_expression_every_element(ctx):
    """e_new = e + (p_new - e) * (1.f - decay) in f32 (include/svg_hip.h), against the same expression in float64 on the library's own
    p_new and previous e.  With c = 1 - decay, the f32 roundings are: p - e (1), 1.f - decay (1), the product (1; none if the
    compiler fuses product and sum), each a factor (1 + d), |d| <= U, on a quantity bounded by c * |p - e| <= c * (|p| + |e|); and
    the sum (1), U of the result.  First order that is U * (3 c (|p| + |e|) + |e_new|); the factor (1 + 4 U) covers the products of
    the four d and the float64 arithmetic of the reference; a product that underflows adds at most the smallest subnormal (sums and
    differences of f32 values are exact down there)."""
    m = make_model("model_10_26", ctx, wide_sd(), **KW)
    m.train()
    m.ema_configure(DECAY)
    d = float(np.float32(DECAY))                                     # the decay as the C argument carries it
    c = 1.0 - d
    prev = ema_of(m)
    start = state_of(m, (_lib.SVG_TENSOR_PARAM,))
    assert same_bits(prev, {k: v[0] for k, v in start.items()})      # before the first step: the parameters, bit for bit
    checked = 0
    for step in range(3):
        m.training_loss(cfg_of(F, FEAT, MIX, seed=step), batch(3, 40 + step).cuda(), backward=1)
        if step == 1:
            m.adam_step(1e-3)                                        # both kernels carry the statement
        else:
            m.optim_step(1e-3, weight_decay=0.01, decoupled=True)
        now, params = ema_of(m), state_of(m, (_lib.SVG_TENSOR_PARAM,))
        moved = 0
        for k in now:
            p = params[k][0].numpy().astype(np.float64)
            e0 = prev[k].numpy().astype(np.float64)
            e1 = now[k].numpy().astype(np.float64)
            ref = e0 + (p - e0) * c
            bound = U * (3.0 * c * (np.abs(p) + np.abs(e0)) + np.abs(ref)) * (1.0 + 4.0 * U) + DENORM
            err = np.abs(e1 - ref)
            worst = int(np.argmax(err - bound))
            assert err.flat[worst] <= bound.flat[worst], (step, k, worst, float(err.flat[worst]), float(bound.flat[worst]))
            checked += err.size
            moved += int(np.count_nonzero(e1 != e0))
        assert moved > 0
        prev = now
    assert checked == 3 * sum(v.numel() for v in prev.values())      # none left out


# ---- 4. nothing moves when it is off ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["adam_step", "optim_step"])
def test_parameters_and_moments_do_not_depend_on_ema(ctx, path):
    sd = wide_sd()

    def step(m):
        if path == "adam_step":
            m.adam_step(1e-3)
        else:
            m.optim_step(1e-3, weight_decay=0.01, decoupled=True, max_grad_norm=0.5, grad_scale=0.5)

    def run(mode):
        m = make_model("model_10_26", ctx, sd, **KW)                 # a new module re-uploads: a fresh training state
        m.train()
        if mode != "never":
            m.ema_configure(DECAY)
        kept = None
        for i in range(3):
            m.training_loss(cfg_of(F, FEAT, MIX, seed=i), batch(2, 60 + i).cuda(), backward=1)
            step(m)
            if mode == "switched off" and i == 0:
                m.ema_configure(0.0)
                kept = ema_of(m)
        if mode == "never":
            with pytest.raises(ValueError, match="no averaged weights"):
                ema_of(m)
        return state_of(m), (ema_of(m) if mode != "never" else None), kept

    never, on, off = run("never"), run("on"), run("switched off")
    assert same_bits(on[0], never[0]) and same_bits(off[0], never[0])
    assert not same_bits(never[0], {k: (sd[k],) * 3 for k in never[0]})
    # decay 0 keeps the buffers and their last values: those of the one step taken with the updates on
    assert same_bits(off[1], off[2])
    assert not same_bits(off[1], on[1])
    assert not same_bits(on[1], {k: v[0] for k, v in on[0].items()})


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------
def test_refused_calls_change_nothing(ctx):
    m = make_model("model_10_26", ctx, tiny_sd(), **TINY)
    m.train()
    m.training_loss(cfg_of(F, FEAT, MIX), batch(2, 11).cuda(), backward=1)
    name = "transformer.encoder.layers.0.linear1.weight"
    like = dict(m.named_parameters())[name]
    with pytest.raises(ValueError, match="no averaged weights"):     # before any exist
        ctx.transformer_tensor(name, like, _lib.SVG_TENSOR_EMA)
    m.ema_configure(DECAY)
    m.optim_step(1e-3, weight_decay=0.01)
    before = full_state(m)
    assert before[2] == 1
    ones = torch.ones_like(like).cpu()
    bad = [("kind PARAM", lambda: ctx.transformer_set_tensor(name, ones, _lib.SVG_TENSOR_PARAM), "cannot be set"),
           ("kind GRAD", lambda: ctx.transformer_set_tensor(name, ones, _lib.SVG_TENSOR_GRAD), "cannot be set"),
           ("kind 9", lambda: ctx.transformer_set_tensor(name, ones, 9), "cannot be set"),
           ("unknown name", lambda: ctx.transformer_set_tensor("transformer.nothing.weight", ones, _lib.SVG_TENSOR_EXP_AVG), "no trained tensor"),
           ("the buffer that is no parameter", lambda: ctx.transformer_set_tensor("positional_encoder.pos_encoding", ones, _lib.SVG_TENSOR_EMA), "no trained tensor"),
           ("wrong numel", lambda: ctx.transformer_set_tensor(name, ones.flatten()[:-1], _lib.SVG_TENSOR_EXP_AVG_SQ), "elements"),
           ("wrong numel, EMA", lambda: ctx.transformer_set_tensor(name, torch.ones(3), _lib.SVG_TENSOR_EMA), "elements"),
           ("null data", lambda: ctx.check(ctx.lib.svg_transformer_set_tensor(ctx.h, _lib.SVG_TENSOR_EMA, name.encode(), None, like.numel(), None), "set"), "null"),
           ("null name", lambda: ctx.check(ctx.lib.svg_transformer_set_tensor(ctx.h, _lib.SVG_TENSOR_EMA, None, ones.data_ptr(), like.numel(), None), "set"), "null"),
           ("decay -0.1", lambda: m.ema_configure(-0.1), "decay"),
           ("decay 1.0", lambda: m.ema_configure(1.0), "decay"),
           ("decay 1.5", lambda: m.ema_configure(1.5), "decay"),
           ("decay nan", lambda: m.ema_configure(float("nan")), "decay"),
           ("step -1", lambda: ctx.transformer_set_optim_step_count(-1), "step"),
           ("step 2^31", lambda: ctx.transformer_set_optim_step_count(2 ** 31), "step")]
    for label, call, word in bad:
        raised = None
        try:
            call()
        except ValueError as e:
            raised = str(e)
        assert raised is not None, "accepted: " + label
        assert word in raised, (label, raised)
        assert same_full(full_state(m), before), label
    # the updates are still on and the counter did not move: the next step is step 2 and moves the averaged weights
    m.training_loss(cfg_of(F, FEAT, MIX), batch(2, 12).cuda(), backward=1)
    m.optim_step(1e-3, weight_decay=0.01)
    after = full_state(m)
    assert after[2] == 2 and not same_bits(after[1], before[1])
    # accepted: a moment and the counter, set and read back
    ctx.transformer_set_tensor(name, ones, _lib.SVG_TENSOR_EXP_AVG_SQ)
    ctx.transformer_set_optim_step_count(7)
    assert torch.equal(ctx.transformer_tensor(name, like, _lib.SVG_TENSOR_EXP_AVG_SQ), ones) and ctx.transformer_optim_step_count() == 7


# ---- 6. trainer, end to end ---------------------------------------------------------------------------------------------------------
FLAGS = ["--lr_schedule", "linear", "--warmup_steps", "2", "--ema_decay", "0.9", "--grad_accum", "2", "--clip_grad_norm", "1.0",
         "--optimizer", "adamw"]


class Latents:
    """stands for SDUtils.encode_batch (which samples the VAE posterior): the loader's entries are the encoded batches already"""

    def encode_batch(self, batch, use_sos=True):
        return batch


def _trainer(path, monkeypatch, flags):
    """the pattern of tests/test_train_optim_gpu._trainer with the fixed encoder instead of the synthetic SD networks"""
    from sd_video_gen_amd import trainer as T
    os.makedirs(path, exist_ok=True)
    monkeypatch.chdir(path)
    svg_config.set_args(["--dataset", "ball", "--config", "model_10_26"] + flags)
    tr = T.Trainer(sd_utils=Latents())
    logs = []
    tr.log = logs.append
    return T, tr, logs, _lib.Context(0), svg_config.parse_config_args()[1]


def test_trainer_stop_and_continue_equals_the_uninterrupted_run(tmp_path, monkeypatch):
    from sd_video_gen_amd.transformer import Transformer
    train = [(None, batch(2, 300 + i)) for i in range(3)]               # three batches, two per step: a ragged tail every epoch
    val = [(None, batch(2, 310))]
    lr, epochs = 2e-3, 2
    torch.manual_seed(21)
    sd = {k: v.detach().clone() for k, v in Transformer(dropout_p=0.1, **TINY).state_dict().items()}

    def run(path, flags, first_run_epochs):
        T, tr, logs, c, args = _trainer(path, monkeypatch, flags)
        model = Transformer(dropout_p=0.1, **TINY).use_context(c)
        if not args.resume:
            model.load_state_dict(sd)
            tr.seed = 1000
        loss_fn = tr.criterion(use_mse=True, use_L1=False, use_gdl=True, lambda_gdl=1, alpha=2, use_contrastive=True, lambda_contrastive=0.05)
        opt, scheduler, first_epoch, best_t, best_v = T.prepare_run(tr, args, model, lr, epochs, len(train))
        assert type(opt) is T.AdamW and scheduler.total_steps == 4
        tr.run_epochs(args, model, opt, scheduler, loss_fn, train, val, 3, first_run_epochs, first_epoch, best_t, best_v)
        return tr, logs, first_epoch

    tr_a, logs_a, _ = run(tmp_path / "a", FLAGS, 2)
    tr_b, logs_b, _ = run(tmp_path / "b", FLAGS + ["--save_state", "True"], 1)
    stem_b = "model_10_26_%d" % tr_b.index
    state = torch.load(tmp_path / "b" / "checkpoints" / (stem_b + "_state.pt"), weights_only=True)
    assert state["epoch"] == 1 and state["optimizer"]["step"] == 2 and state["scheduler"]["last_step"] == 2 and state["seed"] == tr_b.seed
    assert state["hyper"]["optimizer"] == "adamw" and state["hyper"]["accumulate"] == 2 and state["optimizer"]["ema"] is not None
    tr_c, logs_c, first_epoch = run(tmp_path / "b", FLAGS + ["--resume", "True", "--old_name", stem_b + "_test", "--old_state", stem_b + "_state"], 2)
    assert first_epoch == 2 and tr_c.index != tr_b.index

    for suffix in ("_test.pt", "_ema.pt"):
        a = torch.load(tmp_path / "a" / "checkpoints" / ("model_10_26_%d%s" % (tr_a.index, suffix)), weights_only=True)
        b = torch.load(tmp_path / "b" / "checkpoints" / ("model_10_26_%d%s" % (tr_c.index, suffix)), weights_only=True)
        assert a.keys() == b.keys() and all(torch.equal(a[k].cpu(), b[k].cpu()) for k in a), suffix
        one = torch.load(tmp_path / "b" / "checkpoints" / (stem_b + suffix), weights_only=True)
        assert not all(torch.equal(a[k].cpu(), one[k].cpu()) for k in a), suffix                 # the second epoch moved them
        fresh = Transformer(dropout_p=0.1, **TINY)
        fresh.load_state_dict(a)                                        # the averaged weights load like a checkpoint
    test_a = torch.load(tmp_path / "a" / "checkpoints" / ("model_10_26_%d_test.pt" % tr_a.index), weights_only=True)
    ema_a = torch.load(tmp_path / "a" / "checkpoints" / ("model_10_26_%d_ema.pt" % tr_a.index), weights_only=True)
    assert not all(torch.equal(test_a[k].cpu(), ema_a[k].cpu()) for k in test_a)

    strip = lambda recs: [{k: v for k, v in r.items() if k != "seconds"} for r in recs]
    assert len(logs_a) == 6 and len(logs_b) == 3 and len(logs_c) == 3                          # (train, val, epoch) per epoch
    assert strip(logs_a[:3]) == strip(logs_b)
    assert strip(logs_a[3:]) == strip(logs_c)
    # warm-up 2 of 4 steps: the rates are 0, 1/2, 1, 1/2 of the base rate; an epoch logs that of its last step
    assert logs_a[0]["lr"] == lr * 0.5 and logs_a[3]["lr"] == lr * 0.5 and "grad_norm_train" in logs_a[3]
