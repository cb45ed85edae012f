"""CPU: the host side of a run that can be scheduled, stopped and continued — the learning-rate schedule against transformers'
schedules on a torch optimizer, where the trainer's loop steps it, the new flags, and the training-state file through a stub model.
The library side (moments, step count, averaged weights) is tests/test_train_resume_gpu.py."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sd_video_gen_amd import config as svg_config  # noqa: E402
from test_train_optim_cpu import BASE, StubModel, make_trainer  # noqa: E402


class Opt:
    """what a WarmupSchedule needs of an optimizer"""

    def __init__(self, lr):
        self.lr = lr


# ---- the schedule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["linear", "cosine"])
@pytest.mark.parametrize("warmup, total", [(0, 10), (3, 10), (10, 10), (12, 10), (0, 0), (15, 40)])
def test_schedule_is_the_transformers_schedule_at_every_step(kind, warmup, total):
    import transformers
    from sd_video_gen_amd import trainer as T
    base = 3e-4
    ref_opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=base)
    make = {"linear": transformers.get_linear_schedule_with_warmup, "cosine": transformers.get_cosine_schedule_with_warmup}[kind]
    ref = make(ref_opt, warmup, total)
    opt = Opt(base)
    mine = T.WarmupSchedule(opt, kind, warmup, total)
    seen = []
    for step in range(max(total, warmup) + 3):                          # and past the end: the rate stays at (or returns to) its floor
        assert mine.get_last_lr() == [opt.lr]
        # both are base * multiplier(step) with the multiplier a Python float: equal, not close
        assert opt.lr == ref.get_last_lr()[0] == ref_opt.param_groups[0]["lr"], (step, opt.lr, ref.get_last_lr())
        seen.append(opt.lr)
        ref_opt.step()
        ref.step()
        mine.step()
    if warmup > 0:
        assert seen[0] == 0.0
    if 0 < warmup < total:
        assert seen[warmup] == base and max(seen) == base and seen[total] == 0.0
        assert seen[1] == base * (1.0 / warmup)


def test_schedule_state_round_trip_and_argument_checks():
    from sd_video_gen_amd import trainer as T
    a_opt, b_opt = Opt(1e-3), Opt(5.0)
    a = T.WarmupSchedule(a_opt, "cosine", 3, 20)
    for _ in range(7):
        a.step()
    sd = a.state_dict()
    assert sd == {"kind": "cosine", "warmup_steps": 3, "total_steps": 20, "base_lr": 1e-3, "last_step": 7}
    b = T.WarmupSchedule(b_opt, "linear", 0, 1)
    b.load_state_dict(sd)
    assert b_opt.lr == a_opt.lr and b.state_dict() == sd                # the position and the rate it implies
    for _ in range(15):
        a.step()
        b.step()
        assert b_opt.lr == a_opt.lr
    for bad in (("step", 0, 10), ("linear", -1, 10), ("cosine", 0, -1)):
        with pytest.raises(ValueError):
            T.WarmupSchedule(Opt(1.0), *bad)


# ---- where the loop steps it ------------------------------------------------------------------------------------------------------
class CountingSchedule:
    def __init__(self, opt, events):
        self.opt, self.events, self.steps = opt, events, 0

    def step(self):
        self.steps += 1
        self.events.append(("sched", self.steps))
        self.opt.lr = 1e-3 / (1 + self.steps)

    def get_last_lr(self):
        return [self.opt.lr]


def test_scheduler_is_stepped_once_per_optimizer_step_including_the_ragged_tail(tmp_path, monkeypatch):
    T, tr, logs = make_trainer(tmp_path, monkeypatch, ["--grad_accum", "3"])
    model = StubModel()
    opt = T.make_optimizer(svg_config.parse_config_args()[1], model, 1e-3)
    sched = CountingSchedule(opt, model.events)
    loss_fn = tr.criterion(use_mse=True, use_L1=False, use_gdl=True, use_contrastive=False)
    tr.train_loop(model, opt, sched, loss_fn, [(None, None)] * 7, 3)
    assert sched.steps == 3                                              # 3 + 3 + 1 batches
    kinds = [e[0] for e in model.events]
    assert kinds == ["loss"] * 3 + ["step", "sched"] + ["loss"] * 3 + ["step", "sched"] + ["loss", "step", "sched"]
    assert logs[0]["lr"] == 1e-3 / 3                                     # the rate the epoch's LAST step used: two scheduler steps behind it
    # the validation loop takes no scheduler and steps nothing
    tr.validation_loop(model, loss_fn, [(None, None)] * 2, 3)
    assert sched.steps == 3 and "lr" not in logs[1]


def test_no_scheduler_leaves_the_rate_and_the_log_alone(tmp_path, monkeypatch):
    T, tr, logs = make_trainer(tmp_path, monkeypatch, ["--grad_accum", "2"])
    _, args = svg_config.parse_config_args()
    model = StubModel()
    opt = T.make_optimizer(args, model, 1e-3)
    assert T.make_scheduler(args, opt, 5, 7) is None and opt.lr == 1e-3
    loss_fn = tr.criterion(use_mse=True, use_L1=False, use_gdl=True, use_contrastive=False)
    tr.train_loop(model, opt, None, loss_fn, [(None, None)] * 3, 3)
    assert opt.lr == 1e-3 and "lr" not in logs[0]
    assert set(logs[0]) == {"train_loss", "mse_train", "L1_train", "gdl_train", "contrastive_train"}


def test_make_scheduler_counts_optimizer_steps(tmp_path, monkeypatch):
    T, tr, logs = make_trainer(tmp_path, monkeypatch, ["--grad_accum", "3", "--lr_schedule", "cosine", "--warmup_steps", "4"])
    _, args = svg_config.parse_config_args()
    opt = T.make_optimizer(args, StubModel(), 1e-3)
    s = T.make_scheduler(args, opt, 5, 7)                                # 7 batches in groups of 3: 3 steps an epoch
    assert (s.kind, s.warmup_steps, s.total_steps, s.base_lr) == ("cosine", 4, 15, 1e-3) and opt.lr == 0.0


# ---- flags ----------------------------------------------------------------------------------------------------------------------------
def test_run_flags_and_their_defaults():
    _, args = svg_config.parse_config_args(BASE)
    assert (args.lr_schedule, args.warmup_steps, args.ema_decay, args.save_state, args.old_state) == ("none", 0, 0.0, False, None)
    # and every default that was there before
    assert (args.grad_accum, args.clip_grad_norm, args.weight_decay, args.optimizer) == (1, 0.0, 0.0, "adam")
    assert (args.resume, args.old_name, args.save_best) == (False, "old_name_default", False)
    _, args = svg_config.parse_config_args(BASE + ["--lr_schedule", "cosine", "--warmup_steps", "15", "--ema_decay", "0.999", "--save_state", "True",
                                                   "--resume", "True", "--old_name", "w", "--old_state", "s"])
    assert (args.lr_schedule, args.warmup_steps, args.ema_decay, args.save_state, args.old_state) == ("cosine", 15, 0.999, True, "s")
    assert isinstance(args.warmup_steps, int) and isinstance(args.ema_decay, float)
    with pytest.raises(SystemExit):
        svg_config.parse_config_args(BASE + ["--lr_schedule", "step"])


def test_old_state_needs_resume():
    with pytest.raises(ValueError, match="--resume"):
        svg_config.parse_config_args(BASE + ["--old_state", "model_10_26_0_state"])
    with pytest.raises(ValueError, match="--resume"):
        svg_config.parse_config_args(BASE + ["--old_name", "model_10_26_0_test", "--old_state", "model_10_26_0_state"])


# ---- the training-state file ----------------------------------------------------------------------------------------------------------
class StatefulStub(StubModel):
    """the stub with an optimizer state: two parameters, moments that count the steps taken"""
    NAMES = ("embedding.weight", "out.bias")

    def __init__(self):
        super().__init__()
        self.steps, self.ema_decay, self.loaded = 0, 0.0, None

    def adam_step(self, *a, **k):
        self.steps += 1
        super().adam_step(*a, **k)

    def optim_step(self, *a, **k):
        self.steps += 1
        return super().optim_step(*a, **k)

    def optimizer_state(self):
        t = lambda x: {n: torch.full((2, 3), float(x)) for n in self.NAMES}
        return {"step": self.steps, "exp_avg": t(self.steps), "exp_avg_sq": t(self.steps ** 2), "ema": t(0.5) if self.ema_decay > 0 else None}

    def load_optimizer_state(self, state):
        self.loaded = state
        self.steps = state["step"]
        self.events.append(("load_optimizer_state", state["step"]))

    def load_state_dict(self, sd):
        self.events.append(("load_state_dict", sorted(sd)))

    def state_dict(self):
        return {n: torch.full((2, 3), float(self.steps)) for n in self.NAMES}

    def ema_configure(self, decay):
        self.ema_decay = decay
        self.events.append(("ema_configure", decay))

    def ema_state_dict(self):
        return {n: torch.full((2, 3), 0.5) for n in self.NAMES}


def test_state_file_round_trips_and_the_next_run_continues(tmp_path, monkeypatch):
    flags = ["--grad_accum", "2", "--clip_grad_norm", "1.0", "--optimizer", "adamw", "--lr_schedule", "linear", "--warmup_steps", "2", "--ema_decay", "0.9"]
    T, tr, logs = make_trainer(tmp_path, monkeypatch, flags + ["--save_state", "True"])
    _, args = svg_config.parse_config_args()
    model = StatefulStub()
    loader = [(None, None)] * 3
    opt, sched, first_epoch, best_t, best_v = T.prepare_run(tr, args, model, 1e-3, 3, len(loader))
    assert first_epoch == 1 and (best_t, best_v) == (1e10, 1e10) and sched.total_steps == 6
    assert model.events == [("ema_configure", 0.9)]
    loss_fn = tr.criterion(use_mse=True, use_L1=False, use_gdl=True, use_contrastive=False)
    tr.seed = 77
    tr.run_epochs(args, model, opt, sched, loss_fn, loader, loader[:1], 3, 2)            # epochs 1 and 2 of 3
    stem = "model_10_26_%d" % tr.index
    assert sorted(os.listdir("checkpoints")) == [stem + s for s in ("_ema.pt", "_state.pt", "_test.pt")]
    state = torch.load("./checkpoints/" + stem + "_state.pt", weights_only=True)        # plain tensors, numbers and strings
    assert state["epoch"] == 2 and state["seed"] == 77 + 2 * 4 and state["optimizer"]["step"] == 4
    assert state["scheduler"] == sched.state_dict() and state["scheduler"]["last_step"] == 4
    assert state["hyper"] == {"optimizer": "adamw", "lr": opt.lr, "beta1": 0.9, "beta2": 0.999, "eps": 1e-8, "weight_decay": 0.0,
                              "max_grad_norm": 1.0, "accumulate": 2}
    assert (state["best_train_loss"], state["best_val_loss"]) == (1e10, 1e10)            # --save_best is off: nothing tracks them
    assert torch.equal(state["optimizer"]["exp_avg_sq"]["out.bias"], torch.full((2, 3), 16.0)) and state["optimizer"]["ema"] is not None
    assert torch.equal(torch.load("./checkpoints/" + stem + "_ema.pt", weights_only=True)["out.bias"], torch.full((2, 3), 0.5))

    # the continued run: the weights, then the state, then the averaging; it starts at epoch 3 where the first one stopped
    T2, tr2, logs2 = make_trainer(tmp_path, monkeypatch, flags + ["--resume", "True", "--old_name", stem + "_test", "--old_state", stem + "_state"])
    _, args2 = svg_config.parse_config_args()
    again = StatefulStub()
    opt2, sched2, first_epoch, best_t, best_v = T2.prepare_run(tr2, args2, again, 1e-3, 3, len(loader))
    assert [e[0] for e in again.events] == ["load_state_dict", "load_optimizer_state", "ema_configure"]
    assert first_epoch == 3 and tr2.seed == state["seed"] and again.steps == 4
    assert sched2.state_dict() == sched.state_dict() and opt2.lr == opt.lr
    assert torch.equal(again.loaded["exp_avg"]["embedding.weight"], torch.full((2, 3), 4.0))
    tr2.run_epochs(args2, again, opt2, sched2, loss_fn, loader, loader[:1], 3, 3, first_epoch, best_t, best_v)
    assert [r["epoch"] for r in logs2 if "epoch" in r] == [3] and sched2.last_step == 6 and opt2.lr == 0.0


def test_save_best_tracks_the_best_losses_into_the_state(tmp_path, monkeypatch):
    T, tr, logs = make_trainer(tmp_path, monkeypatch, ["--save_best", "True", "--save_state", "True"])
    _, args = svg_config.parse_config_args()
    model = StatefulStub()
    opt, sched, first_epoch, best_t, best_v = T.prepare_run(tr, args, model, 1e-3, 1, 2)
    assert sched is None and model.events == []
    loss_fn = tr.criterion(use_mse=True, use_L1=False, use_gdl=True, use_contrastive=False)
    assert tr.run_epochs(args, model, opt, sched, loss_fn, [(None, None)] * 2, [(None, None)], 3, 1) == (1.0, 1.0)
    stem = "model_10_26_%d" % tr.index
    state = torch.load("./checkpoints/" + stem + "_state.pt", weights_only=True)
    assert (state["best_train_loss"], state["best_val_loss"], state["scheduler"]) == (1.0, 1.0, None)
    assert sorted(os.listdir("checkpoints")) == [stem + s for s in ("_state.pt", "_test.pt", "_train.pt")]      # no averaged weights asked for
