"""Host side of the training step — mirror of the reference's ``trainers/trainer.py`` (Trainer: :39-300, main: :303-480).

What runs where: ``encode_batch`` is the HIP VAE encoder of the sampling path (frozen, like the reference's SD models); the
latent Transformer's train-mode forward, the criterion, the backward pass and Adam run inside libsvg_hip.so
(``svg_transformer_loss`` / ``svg_transformer_adam_step``, include/svg_hip.h) on the library's copy of the weights.  The
objects the reference's loop passes around keep their roles:

  * ``criterion(...)``      trainer.py:91-109 — returns the loss description the library evaluates (a ``Criterion``), with the
                            same keyword arguments; the invalid use_mse + use_L1 combination prints and returns None like there
  * ``Adam(model, lr)``     stands for ``optim.Adam(model.parameters(), lr=lr)`` (trainer.py:365): ``zero_grad()`` / ``step()``;
                            ``AdamW`` for ``optim.AdamW``.  Both carry what the reference's loop does not have: ``max_grad_norm``
                            (``clip_grad_norm_`` before the step) and ``accumulate`` (micro-batches per optimizer step), see below
  * ``train_loop`` / ``validation_loop`` / ``fit``   trainer.py:111-190, :192-260, :262-273 (same arguments, same returns)
  * ``main()``              trainer.py:303-480 without wandb (absent here): hyper-parameters come from the YAML config
                            (first entry of each list, exactly the values a one-point wandb sweep would deliver), the log is
                            JSON lines on stdout; checkpoints ``./checkpoints/<config>_<index>_{train,test}.pt`` as at :469-480.

Additions (all off by default; the defaults run the reference's loop step for step): ``--grad_accum K`` sums the gradients of K
batches before one optimizer step on their mean (the loss of each micro-batch divided by the number accumulated, as
``(loss / K).backward()`` would; a ragged tail at the end of an epoch is a step of its own), ``--clip_grad_norm X`` clips the
global gradient 2-norm, ``--weight_decay W`` and ``--optimizer adam|adamw`` choose the decay and its form.  The norm, the clip
and the update run in the library (``svg_transformer_optim_step``); with clipping on, the pre-clip norm is read back once per step
and its epoch mean is logged as ``grad_norm_train``.

The run around the optimizer (again all off by default): ``--lr_schedule linear|cosine --warmup_steps N`` drives ``opt.lr`` with a
``WarmupSchedule`` (the multipliers of transformers' ``get_linear_schedule_with_warmup`` / ``get_cosine_schedule_with_warmup``,
stepped once per optimizer step: the ``scheduler.step()`` the reference left commented at trainer.py:166; its sketch at :367),
``--ema_decay D`` keeps averaged weights inside the update kernel and writes them as ``<stem>_ema.pt`` beside ``<stem>_test.pt``,
``--save_state True`` writes ``<stem>_state.pt`` after every epoch (Adam moments, step count, averaged weights, scheduler
position, dropout seed, finished epoch, best losses: plain tensors and numbers, ``torch.load(weights_only=True)``), and
``--resume True --old_name W --old_state S`` continues from both files at the next epoch.  Given the same batches the continued
run computes what the uninterrupted one would, bit for bit; the sampler's shuffling order is not restored.

Deviations, logging only: the per-term losses logged are those of the F predicted positions (the reference logs the GDL of all
positions, trainer.py:176) and the contrastive term is reported directly instead of as ``loss - mse - gdl`` (:178).
"""
import contextlib
import json
import math
import os
import time

import torch

from . import _lib
from .config import parse_config_args


class Criterion:
    """the loss of trainer.py:91-109 as the library evaluates it: w_mse*MSE + w_l1*L1 + w_gdl*GDL(alpha) + w_con*BiPatchNCE(tau)"""

    def __init__(self, use_mse, use_L1, use_gdl, lambda_gdl, alpha, use_contrastive, temperature, lambda_contrastive, feat):
        self.w_mse = float(bool(use_mse))
        self.w_l1 = float(bool(use_L1))
        self.w_gdl = float(bool(use_gdl)) * float(lambda_gdl)
        self.alpha = float(alpha)
        self.w_contrastive = float(bool(use_contrastive)) * float(lambda_contrastive)
        self.temperature = float(temperature)
        self.feat = int(feat)

    def cfg(self, frames_to_predict, dropout_p=0.0, seed=0):
        return _lib.TrainCfg(frames_to_predict=int(frames_to_predict), feat_h=self.feat, feat_w=self.feat, w_mse=self.w_mse, w_l1=self.w_l1,
                             w_gdl=self.w_gdl, gdl_alpha=self.alpha, w_contrastive=self.w_contrastive, temperature=self.temperature,
                             dropout_p=float(dropout_p), seed=int(seed) & (2 ** 64 - 1))


class Adam:
    """``optim.Adam(model.parameters(), lr=lr, weight_decay=weight_decay)`` for a model whose gradients live in the library
    (trainer.py:365).  max_grad_norm > 0: ``clip_grad_norm_(model.parameters(), max_grad_norm)`` in front of every step;
    accumulate: the trainer's loop calls ``step(n)`` once per `accumulate` batches, n = the number of micro-batches summed."""
    decoupled = False       # weight decay as an L2 term of the gradient

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_grad_norm=0.0, accumulate=1):
        if weight_decay < 0 or max_grad_norm < 0 or int(accumulate) < 1:
            raise ValueError("weight_decay and max_grad_norm must be >= 0 and accumulate >= 1")
        self.model, self.lr, self.betas, self.eps = model, lr, betas, eps
        self.weight_decay, self.max_grad_norm, self.accumulate = float(weight_decay), float(max_grad_norm), int(accumulate)
        self.grad_norm = None       # pre-clip norm of the last step (clipping on only: reading it is a synchronisation)

    def zero_grad(self):
        pass            # svg_transformer_loss(backward=1) overwrites the gradients: zero_grad + backward in one

    def step(self, n=1):
        """n: micro-batches whose gradients were summed since the last step (the update sees their mean)"""
        if n == 1 and self.weight_decay == 0.0 and self.max_grad_norm == 0.0:
            self.model.adam_step(self.lr, self.betas, self.eps)
            return
        self.grad_norm = self.model.optim_step(self.lr, self.betas, self.eps, weight_decay=self.weight_decay, decoupled=self.decoupled,
                                               max_grad_norm=self.max_grad_norm, grad_scale=1.0 / n, read_norm=self.max_grad_norm > 0)


class AdamW(Adam):
    """``optim.AdamW(model.parameters(), lr=lr)``: decoupled weight decay, torch's default 1e-2."""
    decoupled = True

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_grad_norm=0.0, accumulate=1):
        super().__init__(model, lr, betas, eps, weight_decay, max_grad_norm, accumulate)


class WarmupSchedule:
    """Learning-rate schedule on ``opt.lr`` with the members of a torch scheduler: linear warm-up from 0 over `warmup_steps`, then
    linear decay to 0 at `total_steps` (kind "linear": the multiplier of transformers.get_linear_schedule_with_warmup) or half a
    cosine (kind "cosine": get_cosine_schedule_with_warmup, num_cycles = 0.5).  Like torch's LambdaLR it applies the multiplier of
    step 0 when it is created; ``step()`` goes behind every optimizer step."""

    def __init__(self, opt, kind, warmup_steps, total_steps):
        if kind not in ("linear", "cosine"):
            raise ValueError("schedule kind must be 'linear' or 'cosine'")
        if int(warmup_steps) < 0 or int(total_steps) < 0:
            raise ValueError("warmup_steps and total_steps must be >= 0")
        self.opt, self.kind, self.warmup_steps, self.total_steps = opt, kind, int(warmup_steps), int(total_steps)
        self.base_lr = float(opt.lr)
        self.last_step = 0
        opt.lr = self.base_lr * self.multiplier(0)

    def multiplier(self, step):
        if step < self.warmup_steps:
            return float(step) / float(max(1, self.warmup_steps))
        if self.kind == "linear":
            return max(0.0, float(self.total_steps - step) / float(max(1, self.total_steps - self.warmup_steps)))
        progress = float(step - self.warmup_steps) / float(max(1, self.total_steps - self.warmup_steps))
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * 0.5 * 2.0 * progress)))

    def step(self):
        self.last_step += 1
        self.opt.lr = self.base_lr * self.multiplier(self.last_step)

    def get_last_lr(self):
        return [self.opt.lr]

    def state_dict(self):
        return {"kind": self.kind, "warmup_steps": self.warmup_steps, "total_steps": self.total_steps, "base_lr": self.base_lr,
                "last_step": self.last_step}

    def load_state_dict(self, sd):
        if sd["kind"] not in ("linear", "cosine"):
            raise ValueError("schedule kind must be 'linear' or 'cosine'")
        self.kind, self.warmup_steps, self.total_steps = sd["kind"], int(sd["warmup_steps"]), int(sd["total_steps"])
        self.base_lr, self.last_step = float(sd["base_lr"]), int(sd["last_step"])
        self.opt.lr = self.base_lr * self.multiplier(self.last_step)


class Trainer:
    def __init__(self, sd_utils=None):
        self.config, self.args = parse_config_args()
        os.makedirs("./checkpoints", exist_ok=True)
        # trainer.py:43: the run index counts the checkpoints that carry this config's name
        self.index = len([name for name in os.listdir("./checkpoints") if self.args.config in name])
        self.device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
        if sd_utils is None:
            from .sd_utils import SDUtils
            sd_utils = SDUtils()
        self.sd_utils = sd_utils
        self.SOS_token = torch.ones((1, 1, self.config.FRAME_SIZE ** 2 // 64 * 4), dtype=torch.float32, device=self.device) * 2
        # dropout: one fresh seed per training iteration.  The masks are a pure function of (seed, site, element), so the starting
        # point carries the entropy: torch's initial seed (torch.manual_seed makes a run reproducible, as in the reference), the
        # rank and the run index — a --resume run, the next sweep point and every replica rank get their own mask sequence
        self.seed = (int(torch.initial_seed()) * 1000003 + int(os.environ.get("RANK", "0")) * 7919 + self.index * 104729) & (2 ** 62 - 1)
        self._stream = torch.cuda.Stream() if torch.cuda.is_available() else None   # capturable: the library replays a step as one hipGraph
        self.log = lambda rec: print(json.dumps(rec), flush=True)

    def criterion(self, use_mse=True, use_L1=False, use_gdl=True, lambda_gdl=1, alpha=2, use_contrastive=True, temperature=0.07,
                  lambda_contrastive=0.1):
        if use_mse and use_L1:
            print("Invalid loss function combination")      # trainer.py:107-109
            return None
        return Criterion(use_mse, use_L1, use_gdl, lambda_gdl, alpha, use_contrastive, temperature, lambda_contrastive,
                         self.config.FRAME_SIZE // 8)

    def _on_stream(self):
        """the capturable side stream of the training step (a stub model on a host without a GPU runs without one)"""
        return torch.cuda.stream(self._stream) if self._stream is not None else contextlib.nullcontext()

    def _loop(self, model, loss_fn, dataloader, frames_to_predict, opt, scheduler=None):
        sums = {"total": 0.0, "mse": 0.0, "l1": 0.0, "gdl": 0.0, "contrastive": 0.0}
        n = 0
        train = opt is not None
        accumulate = max(1, int(getattr(opt, "accumulate", 1))) if train else 1
        pending = 0                    # micro-batches whose gradients are summed in the library and not yet applied
        norms, lrs = [], []
        for index_list, batch in dataloader:
            new_batch = self.sd_utils.encode_batch(batch, use_sos=True)                  # trainer.py:123
            new_batch = torch.as_tensor(new_batch).to(self.device)
            self.seed += 1                                                                 # every micro-batch: its own dropout masks
            cfg = loss_fn.cfg(frames_to_predict, model.positional_encoder.dropout_p if train else 0.0, self.seed)
            if train and pending == 0:
                opt.zero_grad()
            if self._stream is not None:
                torch.cuda.current_stream().synchronize()                                  # the encoded batch is ready
            with self._on_stream():
                # :141-145 (+ loss.backward(), :164); the first micro-batch of a step overwrites the gradients, the others add
                terms = model.training_loss(cfg, new_batch, backward=(1 if pending == 0 else _lib.SVG_BACKWARD_ACCUMULATE) if train else 0)
                pending += 1
                if train and pending == accumulate:
                    pending = self._step(opt, pending, norms, scheduler, lrs)              # :165, :166
            if self._stream is not None:
                self._stream.synchronize()
            for k in sums:
                sums[k] += terms[k]
            n += 1
        if train and pending:                                                              # ragged tail of the epoch: a step of its own
            with self._on_stream():
                pending = self._step(opt, pending, norms, scheduler, lrs)
            if self._stream is not None:
                self._stream.synchronize()
        avg = {k: v / max(n, 1) for k, v in sums.items()}
        if norms:
            avg["grad_norm"] = sum(norms) / len(norms)
        if lrs:
            avg["lr"] = lrs[-1]
        return avg

    @staticmethod
    def _step(opt, n, norms, scheduler=None, lrs=None):
        """one optimizer step on the mean of the n accumulated micro-batch gradients -> 0 (nothing pending); a scheduler is stepped
        once behind it (trainer.py:166) and the rate the step used is noted"""
        if scheduler is not None and lrs is not None:
            lrs.append(opt.lr)
        if getattr(opt, "accumulate", 1) > 1:
            opt.step(n)
        else:
            opt.step()
        if getattr(opt, "max_grad_norm", 0.0) > 0 and getattr(opt, "grad_norm", None) is not None:
            norms.append(opt.grad_norm)
        if scheduler is not None:
            scheduler.step()
        return 0

    def train_loop(self, model, opt, scheduler, loss_fn, dataloader, frames_to_predict):
        model.train()
        avg = self._loop(model, loss_fn, dataloader, frames_to_predict, opt, scheduler)
        rec = {"train_loss": avg["total"], "mse_train": avg["mse"], "L1_train": avg["l1"], "gdl_train": avg["gdl"],
               "contrastive_train": avg["contrastive"]}
        if "grad_norm" in avg:
            rec["grad_norm_train"] = avg["grad_norm"]          # pre-clip, mean over the epoch's optimizer steps (clipping on only)
        if "lr" in avg:
            rec["lr"] = avg["lr"]                              # the rate of the epoch's last optimizer step (with a scheduler only)
        self.log(rec)
        return avg["total"]

    def validation_loop(self, model, loss_fn, dataloader, frames_to_predict):
        model.eval()
        avg = self._loop(model, loss_fn, dataloader, frames_to_predict, None)
        self.log({"val_loss": avg["total"], "mse_val": avg["mse"], "L1_val": avg["l1"], "gdl_val": avg["gdl"],
                  "contrastive_val": avg["contrastive"]})
        return avg["total"]

    def fit(self, model, opt, scheduler, loss_fn, train_dataloader, val_dataloader, frames_to_predict):
        print("Training and validating model")
        train_loss = self.train_loop(model, opt, scheduler, loss_fn, train_dataloader, frames_to_predict)
        validation_loss = self.validation_loop(model, loss_fn, val_dataloader, frames_to_predict)
        print(f"Training loss: {train_loss:.4f}")
        print(f"Validation loss: {validation_loss:.4f}")
        return train_loss, validation_loss

    # ---- the training-state file ---------------------------------------------------------------------------------------------
    def training_state(self, model, opt, scheduler, epoch, best_train_loss, best_val_loss):
        """everything beside the weights that the next epoch depends on, as plain tensors / numbers / strings"""
        return {"optimizer": model.optimizer_state(),
                "hyper": dict(self.training_state_hyper(opt), lr=float(opt.lr)),
                "scheduler": scheduler.state_dict() if scheduler is not None else None,
                "seed": int(self.seed), "epoch": int(epoch), "best_train_loss": float(best_train_loss), "best_val_loss": float(best_val_loss)}

    def load_training_state(self, state, model, opt, scheduler):
        """after model.load_state_dict(): puts training_state() back -> (finished epoch, best_train_loss, best_val_loss).  The
        optimizer's hyper-parameters stay those of this run's flags; a difference from the saved ones is printed."""
        model.load_optimizer_state(state["optimizer"])
        if scheduler is not None and state["scheduler"] is not None:
            scheduler.load_state_dict(state["scheduler"])
        elif (scheduler is None) != (state["scheduler"] is None):
            print("note: the saved run %s a learning-rate schedule, this one %s" % (("had", "has none") if scheduler is None else ("had no", "has one")))
        mine = self.training_state_hyper(opt)
        for k, v in state["hyper"].items():
            if k != "lr" and mine.get(k) != v:
                print("note: %s was %s in the saved run and is %s now" % (k, v, mine.get(k)))
        self.seed = int(state["seed"])
        return int(state["epoch"]), float(state["best_train_loss"]), float(state["best_val_loss"])

    @staticmethod
    def training_state_hyper(opt):
        return {"optimizer": "adamw" if opt.decoupled else "adam", "beta1": float(opt.betas[0]), "beta2": float(opt.betas[1]),
                "eps": float(opt.eps), "weight_decay": float(opt.weight_decay), "max_grad_norm": float(opt.max_grad_norm),
                "accumulate": int(opt.accumulate)}

    def run_epochs(self, args, model, opt, scheduler, loss_fn, train_loader, test_loader, frames_to_predict, epochs, first_epoch=1,
                   best_train_loss=1e10, best_val_loss=1e10):
        """epochs first_epoch .. epochs of trainer.py:449-480: fit, log, checkpoints <stem>_{train,test}.pt; with --ema_decay the
        averaged weights as <stem>_ema.pt wherever <stem>_test.pt is written, with --save_state <stem>_state.pt after every epoch"""
        stem = "./checkpoints/" + args.config + "_" + str(self.index)
        tag = args.config + "_" + str(self.index)
        for epoch in range(first_epoch, epochs + 1):
            print("-" * 25, f"Epoch {epoch}", "-" * 25)
            t0 = time.time()
            train_loss, validation_loss = self.fit(model=model, opt=opt, scheduler=scheduler, loss_fn=loss_fn, train_dataloader=train_loader,
                                                   val_dataloader=test_loader, frames_to_predict=frames_to_predict)
            self.log({"epoch": epoch, "seconds": time.time() - t0})
            wrote_test = True
            if args.save_best:                                   # trainer.py:469-477
                wrote_test = False
                if train_loss < best_train_loss:
                    best_train_loss = train_loss
                    torch.save(model.state_dict(), stem + "_train.pt")
                    print("model saved as " + tag + "_train.pt (best train loss)")
                if validation_loss < best_val_loss:
                    best_val_loss = validation_loss
                    torch.save(model.state_dict(), stem + "_test.pt")
                    print("model saved as " + tag + "_test.pt (best test loss)")
                    wrote_test = True
            else:                                                # :478-480
                torch.save(model.state_dict(), stem + "_test.pt")
                print("model saved as " + tag + "_test.pt")
            if wrote_test and args.ema_decay > 0:
                torch.save(model.ema_state_dict(), stem + "_ema.pt")
                print("averaged weights saved as " + tag + "_ema.pt")
            if args.save_state:
                torch.save(self.training_state(model, opt, scheduler, epoch, best_train_loss, best_val_loss), stem + "_state.pt")
                print("training state saved as " + tag + "_state.pt")
        return best_train_loss, best_val_loss


def _first(v):
    return v[0] if isinstance(v, (list, tuple)) else v


def make_loaders(args, config, frames_per_clip, frames_to_predict, stride, batch_size, epoch_ratio, num_workers):
    """trainer.py:372-447.  UCF-101 needs torchvision / PyAV, which this image does not have."""
    from torch.utils.data import DataLoader, RandomSampler
    from .loaders import BouncingBall, Kitti
    if args.dataset == "ball":
        mk = lambda stage: BouncingBall(num_frames=5, stride=stride, dir=args.folder, stage=stage, shuffle=True)
    elif args.dataset == "kitti":
        mk = lambda stage: Kitti(num_frames=(frames_per_clip + frames_to_predict), stride=1, dir=args.folder, stage=stage, shuffle=True)
    elif "ucf" in args.dataset:
        raise RuntimeError("the UCF-101 loader of the reference is torchvision.datasets.UCF101 (PyAV); neither is installed here")
    else:
        raise ValueError("Invalid dataset name")
    out = []
    for stage in ("train", "test"):
        ds = mk(stage)
        sampler = RandomSampler(ds, replacement=False, num_samples=max(1, int(len(ds) * epoch_ratio)))
        out.append(DataLoader(ds, batch_size=batch_size, shuffle=False, sampler=sampler, num_workers=num_workers, pin_memory=True))
    return out


def make_optimizer(args, model, lr):
    """the optimizer the command line asks for: --optimizer adam|adamw, --weight_decay, --clip_grad_norm, --grad_accum (all defaults:
    the reference's ``optim.Adam(model.parameters(), lr=lr)`` stepping on every batch)"""
    return {"adam": Adam, "adamw": AdamW}[args.optimizer](model, lr=lr, weight_decay=args.weight_decay, max_grad_norm=args.clip_grad_norm,
                                                          accumulate=args.grad_accum)


def make_scheduler(args, opt, epochs, batches_per_epoch):
    """--lr_schedule none -> None (the reference's loop); else a WarmupSchedule over epochs x optimizer steps per epoch, an epoch's
    ragged tail being a step of its own (the sketch at trainer.py:367: get_linear_schedule_with_warmup(opt, 15, epochs*len(loader)))"""
    if args.lr_schedule == "none":
        return None
    steps_per_epoch = -(-int(batches_per_epoch) // max(1, int(args.grad_accum)))
    return WarmupSchedule(opt, args.lr_schedule, args.warmup_steps, int(epochs) * steps_per_epoch)


def prepare_run(trainer, args, model, lr, epochs, batches_per_epoch):
    """what stands between a freshly built model and its first epoch: --resume's weights (trainer.py:360-362), the optimizer, the
    schedule, --old_state's training state and the averaged weights -> (opt, scheduler, first epoch, best train loss, best val loss).
    The order is the library's: uploading weights drops its training state, so the weights come first and the state after them."""
    if args.resume:
        model.load_state_dict(torch.load("./checkpoints/" + args.old_name + ".pt", weights_only=True))
    opt = make_optimizer(args, model, lr)
    scheduler = make_scheduler(args, opt, epochs, batches_per_epoch)
    first_epoch, best_train_loss, best_val_loss = 1, 1e10, 1e10
    if args.old_state:
        state = torch.load("./checkpoints/" + args.old_state + ".pt", weights_only=True)
        done, best_train_loss, best_val_loss = trainer.load_training_state(state, model, opt, scheduler)
        first_epoch = done + 1
    if args.ema_decay > 0:                                   # restored averaged weights are kept; otherwise they start as the weights
        model.ema_configure(args.ema_decay)
    return opt, scheduler, first_epoch, best_train_loss, best_val_loss


def main():
    config, args = parse_config_args()
    frames_per_clip, frames_to_predict = _first(config.FRAMES_PER_CLIP), _first(config.FRAMES_TO_PREDICT)
    stride, batch_size, epoch_ratio = _first(config.STRIDE), _first(config.BATCH_SIZE), _first(config.EPOCH_RATIO)
    epochs, lr, num_workers = _first(config.EPOCHS), _first(config.LR), _first(config.NUM_WORKERS)
    from .transformer import Transformer
    trainer = Trainer()
    model = Transformer(num_tokens=0, dim_model=_first(config.DIM_MODEL), num_heads=_first(config.NUM_HEADS),
                        num_encoder_layers=_first(config.NUM_ENCODER_LAYERS), num_decoder_layers=_first(config.NUM_DECODER_LAYERS),
                        dropout_p=_first(config.DROPOUT_P))
    print("number of parameters: ", sum(p.numel() for p in model.parameters() if p.requires_grad))
    loss_fn = trainer.criterion(use_mse=_first(config.USE_MSE), use_L1=_first(getattr(config, "USE_L1", False)), use_gdl=_first(config.USE_GDL),
                                lambda_gdl=_first(config.LAMBDA_GDL), alpha=_first(config.ALPHA),
                                use_contrastive=_first(getattr(config, "USE_CONTRASTIVE", False)),
                                lambda_contrastive=_first(getattr(config, "LAMBDA_CONTRASTIVE", 0.0)))
    if loss_fn is None:
        raise ValueError("Invalid loss function combination")
    train_loader, test_loader = make_loaders(args, config, frames_per_clip, frames_to_predict, stride, batch_size, epoch_ratio, num_workers)
    opt, scheduler, first_epoch, best_train_loss, best_val_loss = prepare_run(trainer, args, model, lr, epochs, len(train_loader))
    trainer.run_epochs(args, model, opt, scheduler, loss_fn, train_loader, test_loader, frames_to_predict, epochs, first_epoch,
                       best_train_loss, best_val_loss)


if __name__ == "__main__":
    main()
