"""``euromillioner train`` / ``predict`` / ``backtest`` (T5 trainers, T6 checkpoints, T4 data parallelism).

The reference has exactly one "training" call site — ``XGBoost.train`` x2 in
``Main.java:128-138`` — and no MLP/RF/DP at all; the north star adds them
(``BASELINE.json``).  This module wires the engines to the config/CLI:

===========  ==============================================  =============================
model        engine (first that applies)                     distributed
===========  ==============================================  =============================
mlp          fused single-launch HIP kernel (62->128->62)     grad all-reduce (C1), RCCL
             -> GEMM trainer (other sizes, GPU)              per-layer async buckets (C1)
             -> DrawMLP + torch Adam (CPU / lags > 1)        GradBucketer hooks (C1), gloo
mlp-wide     GEMM trainer, 62->8192->8192->62                per-layer async buckets (C1)
rf           HIP forest engine / numpy oracle                tree-parallel + all-gather (C5)
gbdt         reference pipeline (XGBoost semantics)          single process
counts       transition-count table: HIP counts + logits     single process
             / numpy specification (the baseline)
===========  ==============================================  =============================

Data parallelism is one process per device (``torchrun``); every rank reads the same
draw sequence and trains on its contiguous shard of the training split; the global
batch ``mlp.batch`` is split evenly across ranks.  MLP checkpoints are DL4J
``ModelSerializer``-layout zips (:mod:`euromillioner_amd.ckpt.modelserializer`)
carrying the Adam state, so ``--resume`` continues exactly.
"""
from __future__ import annotations

import math
import os
import time
from typing import Any, NamedTuple

import numpy as np
import torch

from . import log as L
from .ckpt import modelserializer as MS
from .config import RunConfig
from .data.draws import lag_features, multi_hot, positional_split
from .parallel import dist as D
from .pipeline import date_str, load_draws, next_draw_date, run_reference_pipeline


# ---------------------------------------------------------------------------------------------
# engines: one interface over the three MLP implementations
# ---------------------------------------------------------------------------------------------
class _Engine:
    name = "base"

    def step(self, idx: torch.Tensor | None, offset: int, B: int, global_batch: int) -> torch.Tensor:
        raise NotImplementedError

    def evaluate(self, offset: int, n: int) -> dict:
        raise NotImplementedError

    n_local = 0  # local steps taken (parameter-averaging phase; restored on resume)
    avg_k = 0

    def finish(self) -> None:
        """End of training: with --avg-frequency k, average once more unless the last local step
        just did (Spark's ParameterAveragingTrainingMaster averages at the end of every fit), so the
        final evaluation, the checkpoint and the cross-rank check see one model."""
        if self.avg_k > 0 and self.n_local % self.avg_k != 0:
            self.average_parameters()
            self.n_local = 0

    def average_parameters(self) -> None:
        pass


def _checksum(flat: torch.Tensor) -> torch.Tensor:
    """Order-sensitive integer checksum of a float buffer (bit-exact comparison across ranks)."""
    bits = flat.detach().reshape(-1).view(torch.int32).to(torch.int64)
    w = torch.arange(bits.numel(), device=bits.device, dtype=torch.int64) % 65521 + 1
    return torch.stack([bits.sum(), (bits * w).sum()])


def check_sync(engine: "_Engine", info: D.DistInfo) -> None:
    """Race/desync detector: every rank must hold bit-identical parameters."""
    if not info.is_dist:
        return
    c = _checksum(engine.flat_params())
    if info.backend == "gloo":
        c = c.cpu()
    allc = [torch.zeros_like(c) for _ in range(info.world)]
    torch.distributed.all_gather(allc, c)
    if any(not torch.equal(allc[0], x) for x in allc[1:]):
        raise RuntimeError("data-parallel ranks diverged: parameter checksums differ " +
                           str([x.tolist() for x in allc]))


def _sharded_eval(model, masks, offset: int, n: int) -> dict:
    """C3: each rank scores its slice of the validation range; the model all-reduces the sums."""
    if model.group is None:
        return model.evaluate(masks, n, offset=offset)
    import torch.distributed as dist

    a, b = D.shard_range(n, D.DistInfo(dist.get_rank(model.group), dist.get_world_size(model.group)))
    return model.evaluate(masks, b - a, offset=offset + a)


class _FusedEngine(_Engine):
    """62->128->62 on csrc/mlp_fused.hip + csrc/adam.hip."""

    name = "fused"
    _MAP = {"layers.0.weight": "l1.weight", "layers.0.bias": "l1.bias", "layers.1.weight": "l2.weight",
            "layers.1.bias": "l2.bias"}

    def __init__(self, cfg: RunConfig, info: D.DistInfo, masks: torch.Tensor, sd: dict):
        from .models.mlp import FusedSmallMLP

        m = cfg.mlp
        self.model = FusedSmallMLP(info.device, loss=m.loss, lr=m.lr, betas=tuple(m.betas), eps=m.eps,
                                   weight_decay=m.weight_decay, state_dict={self._MAP[k]: v for k, v in sd.items()},
                                   process_group=info.group, dtype=m.dtype)
        self.masks = masks

    def step(self, idx, offset, B, global_batch):
        return self.model.step(self.masks, B, offset=offset, sidx=idx, global_batch=global_batch)

    def evaluate(self, offset, n):
        return _sharded_eval(self.model, self.masks, offset, n)

    def state_dict(self):
        inv = {v: k for k, v in self._MAP.items()}
        return {inv[k]: v for k, v in self.model.state_dict().items()}

    def optimizer_state(self):
        st = self.model.optimizer_state()
        inv = {v: k for k, v in self._MAP.items()}
        return {"m": {inv[k]: v for k, v in st["m"].items()}, "v": {inv[k]: v for k, v in st["v"].items()},
                "step": st["step"]}

    def load_optimizer_state(self, st):
        self.model.load_optimizer_state({"m": {self._MAP[k]: v for k, v in st["m"].items()},
                                         "v": {self._MAP[k]: v for k, v in st["v"].items()}, "step": st["step"]})

    def broadcast(self):
        self.model.broadcast_parameters()

    def flat_params(self):
        return self.model.params


class _GemmEngine(_Engine):
    """Any 62->...->62 stack on the K1-K3 GEMMs + K10 loss + flat Adam."""

    name = "gemm"

    def __init__(self, cfg: RunConfig, info: D.DistInfo, masks: torch.Tensor, sizes, sd: dict):
        from .models.gemm_mlp import GemmMLPTrainer

        m = cfg.mlp
        self.info = info
        # --avg-frequency k (Spark ParameterAveraging parity): local steps, flat parameter + moment
        # averaging every k steps; otherwise synchronous gradient all-reduce inside the step
        self.avg_k = int(cfg.dist.avg_frequency or 0)
        self.model = GemmMLPTrainer(sizes, info.device, activation=m.activation, loss=m.loss, lr=m.lr,
                                    betas=tuple(m.betas), eps=m.eps, weight_decay=m.weight_decay, state_dict=sd,
                                    process_group=None if self.avg_k > 0 else info.group,
                                    bucket_mb=cfg.dist.bucket_mb, dtype=m.dtype, lags=cfg.data.lags,
                                    comm_dtype=cfg.dist.comm_dtype)
        self.masks = masks
        self.accum = m.accum
        self.n_local = 0

    def step(self, idx, offset, B, global_batch):
        k = self.accum
        gb = B if self.avg_k > 0 else global_batch  # local steps average over the local batch
        if k > 1:  # B consecutive samples as k micro-batches (gradient accumulation)
            out = self.model.step(self.masks, B // k, offset=offset, global_batch=gb, accum=k)
        else:
            out = self.model.step(self.masks, B, offset=offset, sidx=idx, global_batch=gb)
        if self.avg_k > 0:
            self.n_local += 1
            if self.n_local % self.avg_k == 0 and self.info.is_dist:
                self.model.average_parameters(self.info.group)
            if self.info.is_dist:
                out = out.clone()
                torch.distributed.all_reduce(out)
                out /= self.info.world
        return out

    def evaluate(self, offset, n):
        return _sharded_eval(self.model, self.masks, offset, n)

    def state_dict(self):
        return self.model.state_dict()

    def optimizer_state(self):
        return self.model.optimizer_state()

    def load_optimizer_state(self, st):
        self.model.load_optimizer_state(st)

    def broadcast(self):
        self.model.broadcast_parameters(group=self.info.group)

    def flat_params(self):
        return self.model.params

    def average_parameters(self):
        if self.info.is_dist:
            self.model.average_parameters(self.info.group)


class _TorchEngine(_Engine):
    """CPU plumbing engine (BASELINE.json config 1): DrawMLP in PyTorch + torch.optim.Adam + bucketed
    gradient all-reduce overlapped with backward (GradBucketer).  Every GPU run takes the fused or
    the GEMM engine (HIP kernels end to end, fused Adam), lag windows and parameter averaging
    included."""

    name = "torch"

    def __init__(self, cfg: RunConfig, info: D.DistInfo, X: torch.Tensor, Y: torch.Tensor, sizes, sd: dict):
        from .models.mlp import DrawMLP
        from .parallel.buckets import GradBucketer

        m = cfg.mlp
        self.info = info
        # --dtype fp32 on the GPU: plain fp32 layers (the HIP autograd GEMMs are bf16).  The CPU
        # plumbing path (BASELINE config 1) always computes in fp32.
        self.net = DrawMLP(sizes, activation=m.activation, loss=m.loss,
                           use_hip=False if m.dtype == "fp32" else None).to(info.device)
        self.net.load_state_dict(sd)
        self.opt = torch.optim.Adam(self.net.parameters(), lr=m.lr, betas=tuple(m.betas), eps=m.eps,
                                    weight_decay=m.weight_decay)
        self.bucketer = GradBucketer(self.net, cfg.dist.bucket_mb, group=info.group, world=info.world)
        self.avg_k = int(cfg.dist.avg_frequency or 0)
        if self.avg_k > 0:
            self.bucketer.enabled = False  # local steps; parameters are averaged every avg_k steps
        self.n_local = 0
        self.X, self.Y = X, Y
        self.loss_name = m.loss

    def step(self, idx, offset, B, global_batch):
        if idx is not None:
            x, y = self.X[idx.long()], self.Y[idx.long()]
        else:
            x, y = self.X[offset:offset + B], self.Y[offset:offset + B]
        self.bucketer.zero_grad()
        # local mean * (B * world / global_batch): all-reduce of the mean over ranks == global mean
        loss = self.net.loss(self.net(x), y) * (B * self.info.world / global_batch)
        loss.backward()
        self.bucketer.finish()
        self.opt.step()
        self.n_local += 1
        if self.avg_k > 0 and self.n_local % self.avg_k == 0:
            self.average_parameters()
        out = loss.detach().reshape(1)
        if self.info.is_dist:
            torch.distributed.all_reduce(out)
            out /= self.info.world
        return out

    @torch.no_grad()
    def evaluate(self, offset, n):
        from .models.losses import draw_metrics_torch

        a, b = offset, offset + n
        if self.info.is_dist:  # every rank scores its slice of the validation range
            per = D.shard_range(n, self.info)
            a, b = offset + per[0], offset + per[1]
        z = self.net(self.X[a:b])
        r = draw_metrics_torch(z, self.Y[a:b], self.loss_name) if b > a else None
        keys = ("loss", "acc", "acc_thr", "hits_main", "hits_star", "exact", "trivial_acc")
        vec = torch.tensor([r[k] * (b - a) for k in keys] + [b - a] if r else [0.0] * 7 + [0.0], dtype=torch.float64)
        if self.info.is_dist:
            vec = vec.to(self.info.device) if self.info.backend == "nccl" else vec
            torch.distributed.all_reduce(vec)
            vec = vec.cpu()
        cnt = max(float(vec[7]), 1.0)
        out = {k: float(vec[i]) / cnt for i, k in enumerate(keys)}
        out["count"] = int(vec[7])
        return out

    def state_dict(self):
        return {k: v.detach().float().cpu().clone() for k, v in self.net.state_dict().items()}

    def optimizer_state(self):
        m, v, step = {}, {}, 0
        for name, p in self.net.named_parameters():
            st = self.opt.state.get(p, {})
            m[name] = st.get("exp_avg", torch.zeros_like(p)).detach().float().cpu().clone()
            v[name] = st.get("exp_avg_sq", torch.zeros_like(p)).detach().float().cpu().clone()
            step = int(float(st.get("step", 0)))
        return {"m": m, "v": v, "step": step}

    def load_optimizer_state(self, st):
        for name, p in self.net.named_parameters():
            self.opt.state[p] = {"step": torch.tensor(float(st["step"])),
                                 "exp_avg": st["m"][name].to(p.device, p.dtype).clone(),
                                 "exp_avg_sq": st["v"][name].to(p.device, p.dtype).clone()}

    def broadcast(self):
        D.broadcast_module_(self.net, self.info)

    def flat_params(self):
        return torch.cat([p.detach().reshape(-1).float() for p in self.net.parameters()])

    def average_parameters(self):
        """Spark ParameterAveragingTrainingMaster parity: mean of params and Adam moments."""
        if not self.info.is_dist:
            return
        with torch.no_grad():
            for p in self.net.parameters():
                torch.distributed.all_reduce(p.data)
                p.data /= self.info.world
                st = self.opt.state.get(p, {})
                for k in ("exp_avg", "exp_avg_sq"):
                    if k in st:
                        torch.distributed.all_reduce(st[k])
                        st[k] /= self.info.world


# ---------------------------------------------------------------------------------------------
# checkpoints (DL4J ModelSerializer layout)
# ---------------------------------------------------------------------------------------------
def _layer_names(n_layers: int):
    return [(f"layers.{i}.weight", f"layers.{i}.bias") for i in range(n_layers)]


def _flat_from_named(named: dict, n_layers: int) -> np.ndarray:
    layers = [(named[w].numpy().T, named[b].numpy()) for w, b in _layer_names(n_layers)]
    return MS.flatten_params(layers)


def _named_from_flat(flat: np.ndarray, sizes) -> dict:
    out = {}
    for i, (W, b) in enumerate(MS.unflatten_params(np.asarray(flat, np.float32), list(sizes))):
        out[f"layers.{i}.weight"] = torch.from_numpy(np.ascontiguousarray(W.T))
        out[f"layers.{i}.bias"] = torch.from_numpy(np.ascontiguousarray(b))
    return out


def save_mlp_checkpoint(path: str, engine: _Engine, cfg: RunConfig, sizes, step: int, extra: dict | None = None):
    sd = engine.state_dict()
    st = engine.optimizer_state()
    n = len(sizes) - 1
    layers = [(sd[w].numpy().T, sd[b].numpy()) for w, b in _layer_names(n)]
    conf = MS.multilayer_configuration(list(sizes), cfg.mlp.activation, cfg.mlp.loss, cfg.mlp.lr, tuple(cfg.mlp.betas),
                                       cfg.mlp.eps, cfg.mlp.seed)
    meta = {"step": int(step), "adam_step": int(st["step"]), "engine": engine.name, "model": cfg.model,
            "lags": cfg.data.lags, "loss": cfg.mlp.loss, "activation": cfg.mlp.activation, "sizes": list(sizes)}
    meta.update(extra or {})
    tmp = path + ".tmp"
    MS.save(tmp, layers, conf, _flat_from_named(st["m"], n), _flat_from_named(st["v"], n), meta)
    os.replace(tmp, path)  # atomic: a crash never leaves a torn checkpoint


def load_mlp_checkpoint(path: str) -> dict:
    ck = MS.load(path)
    sizes = ck["sizes"]
    out = {"sizes": sizes, "state_dict": _named_from_flat(ck["flat"], sizes), "extra": ck.get("extra", {}),
           "config": ck["config"]}
    if "m" in ck:
        out["opt"] = {"m": _named_from_flat(ck["m"], sizes), "v": _named_from_flat(ck["v"], sizes),
                      "step": int(out["extra"].get("adam_step", out["extra"].get("step", 0)))}
    return out


# ---------------------------------------------------------------------------------------------
# MLP training
# ---------------------------------------------------------------------------------------------
def _export_trace(prof, out_dir: str, rank: int) -> None:
    os.makedirs(out_dir, exist_ok=True)
    prof.export_chrome_trace(os.path.join(out_dir, f"trace_rank{rank}.json"))
    with open(os.path.join(out_dir, f"kernels_rank{rank}.txt"), "w", encoding="utf-8") as f:
        f.write(prof.key_averages().table(sort_by="self_cpu_time_total", row_limit=40))


def _mlp_sizes(cfg: RunConfig) -> tuple:
    hidden = tuple(int(h) for h in cfg.mlp.hidden)
    if cfg.model == "mlp-wide" and hidden == (128,):
        hidden = (8192, 8192)
    return (62 * cfg.data.lags,) + hidden + (62,)


def _fused_shape(cfg: RunConfig, sizes) -> bool:
    """The configurations the fused train kernel covers (62 -> 128 -> 62 relu, no parameter averaging);
    every other stack, lag window or averaging run takes the GEMM engine."""
    return tuple(sizes) == (62, 128, 62) and cfg.mlp.activation == "relu" and not cfg.dist.avg_frequency


def _pick_engine(cfg: RunConfig, info: D.DistInfo, sizes) -> str:
    if info.device.type != "cuda":
        return "torch"  # CPU plumbing path
    if _fused_shape(cfg, sizes):
        return "fused"  # the fused train kernel: bf16 (mlp_fused.hip) or exact fp32 (mlp_fused_f32.hip)
    return "gemm"  # any other stack, lag windows, parameter averaging


def train_mlp(cfg: RunConfig) -> dict:
    log = L.get("Trainer")
    # RCCL at high stream priority only for the GEMM engine's bucketed all-reduces (parallel/dist.py)
    gemm_like = not _fused_shape(cfg, _mlp_sizes(cfg))  # the same predicate as _pick_engine
    info = D.init(cfg.dist.backend, cfg.dist.timeout_s, device=cfg.device, high_priority=gemm_like)
    try:
        return _train_mlp(cfg, info, log)
    finally:
        D.shutdown(info)


def _train_mlp(cfg: RunConfig, info: D.DistInfo, log) -> dict:
    m = cfg.mlp
    sizes = _mlp_sizes(cfg)
    lags = cfg.data.lags
    device_data = cfg.data.source == "device"
    if device_data:  # HBM-resident draws generated on the GPU (csrc/datagen.hip); no host copy
        from .data.device_gen import gb_to_draws, generate_masks

        if info.device.type != "cuda":
            raise ValueError("data.source=device needs a GPU")
        n_draws = int(cfg.data.n_draws) if cfg.data.n_draws else gb_to_draws(cfg.data.device_gb)
        dmasks = generate_masks(n_draws, seed=cfg.data.seed, planted=cfg.data.planted, device=info.device)
        ds = None
        n_samples = n_draws - lags
    else:
        ds = load_draws(cfg)
        n_samples = len(ds) - lags
    if n_samples < 4:
        raise ValueError(f"need more draws than lags+3 (have {n_samples + lags})")
    margin = positional_split(n_samples, cfg.data.train_pct)
    a, b = D.shard_range(margin, info)
    shard = b - a
    if shard < 1:
        raise ValueError("training split smaller than the number of ranks")
    local_b = max(1, min(shard, math.ceil(m.batch / info.world)))
    if m.accum > 1:
        local_b = max(m.accum, local_b // m.accum * m.accum)
    global_b = local_b * info.world
    steps = m.steps if m.epochs is None else int(m.epochs) * math.ceil(shard / local_b)

    resume_path = cfg.ckpt.resume
    if resume_path == "auto":  # restart-safe (torchrun --max-restarts): continue from ckpt.path if present
        resume_path = cfg.ckpt.path if cfg.ckpt.path and os.path.exists(cfg.ckpt.path) else None
    resume = load_mlp_checkpoint(resume_path) if resume_path else None
    if resume is not None:
        if tuple(resume["sizes"]) != tuple(sizes):
            raise ValueError(f"checkpoint sizes {resume['sizes']} != configured {list(sizes)}")
        sd = resume["state_dict"]
    else:
        from .models.mlp import DrawMLP

        sd = DrawMLP(sizes, activation=m.activation, loss=m.loss, seed=m.seed).state_dict()
    kind = _pick_engine(cfg, info, sizes)
    if device_data and kind == "torch":
        raise ValueError("data.source=device feeds the GPU engines")
    if m.accum > 1 and kind != "gemm":
        raise ValueError(f"mlp.accum applies to the GEMM engine (this run uses {kind}); the fused kernel takes "
                         "any batch in one launch")
    dev = info.device
    if kind in ("fused", "gemm"):
        from .models.mlp import FusedSmallMLP

        masks = dmasks if device_data else FusedSmallMLP.prepare(torch.from_numpy(ds.numbers).to(dev))
        engine = _FusedEngine(cfg, info, masks, sd) if kind == "fused" else _GemmEngine(cfg, info, masks, sizes, sd)
        sample_base = 0  # sample i -> masks[i] -> masks[i+1]
    else:
        X, Y = lag_features(ds.numbers, lags)
        engine = _TorchEngine(cfg, info, torch.from_numpy(X).to(dev), torch.from_numpy(Y).to(dev), sizes, sd)
        sample_base = 0
    engine.broadcast()  # C2
    start_step = 0
    if resume is not None:
        start_step = int(resume["extra"].get("step", 0))
        if "opt" in resume:
            engine.load_optimizer_state(resume["opt"])
        engine.n_local = start_step  # keeps the --avg-frequency phase of the interrupted run
        log.info(f"resumed from {resume_path} at step {start_step}")
    log.info(f"mlp {'->'.join(map(str, sizes))} engine={engine.name} device={dev} world={info.world} "
             f"train={margin} (shard {shard}) val={n_samples - margin} batch={global_b} steps={steps}")

    # sample-level shuffles need int32 indices and a host permutation of the shard; device datasets
    # (up to HBM size) and gradient accumulation shuffle whole windows of local_b samples instead
    window_shuffle = device_data or m.accum > 1
    use_perm = m.shuffle and local_b < shard and not window_shuffle
    per_epoch = max(1, shard // local_b)
    wperm, wperm_epoch = None, -1
    perm, perm_epoch = None, -1
    ckpt_path = cfg.ckpt.path
    hist = []
    loss_t = None
    prof = None
    if cfg.log.profile_dir:  # step timeline (chrome trace) for the first profile_steps steps
        from torch.profiler import ProfilerActivity, profile

        acts = [ProfilerActivity.CPU] + ([ProfilerActivity.CUDA] if dev.type == "cuda" else [])
        prof = profile(activities=acts, acc_events=True)  # one cycle: keep its events (and no torch warning)
        prof.__enter__()
    t0 = time.time()
    done = 0
    for step in range(start_step, steps):
        D.maybe_inject_fault(step, info, cfg.dist.fault_at_step, cfg.dist.fault_rank)
        if prof is not None and step == start_step + cfg.log.profile_steps:
            prof.__exit__(None, None, None)
            _export_trace(prof, cfg.log.profile_dir, info.rank)
            prof = None
        idx, off = None, a + sample_base
        if use_perm:  # epoch-keyed permutation: a resumed run sees the same sample order
            epoch, k = divmod(step, per_epoch)
            if epoch != perm_epoch:
                g = np.random.default_rng([m.seed, info.rank, epoch])
                perm = torch.from_numpy((a + g.permutation(shard)).astype(np.int32)).to(dev)
                perm_epoch = epoch
            idx = perm[k * local_b:(k + 1) * local_b]
        elif window_shuffle:
            epoch, k = divmod(step, per_epoch)
            if m.shuffle and epoch != wperm_epoch:
                wperm = np.random.default_rng([m.seed, info.rank, epoch]).permutation(per_epoch)
                wperm_epoch = epoch
            off += int(wperm[k] if m.shuffle else k) * local_b
        loss_t = engine.step(idx, off, local_b, global_b)
        done += 1
        last = step == steps - 1
        if last:
            engine.finish()
        if cfg.dist.check_sync_every and (step + 1) % cfg.dist.check_sync_every == 0:
            check_sync(engine, info)
        if (m.eval_every and (step + 1) % m.eval_every == 0) or last:
            n_val = n_samples - margin if not device_data else min(n_samples - margin, 1 << 24)
            ev = engine.evaluate(margin, n_val) if n_samples > margin else {}
            loss = float(loss_t.reshape(-1)[0].item())
            hist.append({"step": step + 1, "loss": loss, **{f"val_{k}": v for k, v in ev.items()}})
            log.info(f"step {step + 1}/{steps} loss {loss:.5f} val_acc {ev.get('acc', float('nan')):.4f} "
                     f"hits {ev.get('hits_main', float('nan')):.3f}+{ev.get('hits_star', float('nan')):.3f}")
        if ckpt_path and cfg.ckpt.every and (step + 1) % cfg.ckpt.every == 0 and not last:
            # --avg-frequency: rank 0's local parameters and moments are not the model every rank
            # resumes from after a restart, so a checkpoint between averaging points averages first
            # (collective; at fixed steps, so a restarted run and an uninterrupted one take the same
            # averages and stay bit-identical).  Limitation: that extra average is part of
            # the trajectory, so with --avg-frequency k a run with --ckpt-every c (c not a multiple of
            # k) differs from the same run without checkpoints; choose c a multiple of k to keep Spark
            # ParameterAveraging's schedule exactly (tests/test_dist.py
            # test_ckpt_at_averaging_points_keeps_trajectory)
            if engine.avg_k > 0 and engine.n_local % engine.avg_k != 0 and info.is_dist:
                engine.average_parameters()
            if info.rank == 0:
                save_mlp_checkpoint(ckpt_path, engine, cfg, sizes, step + 1)
            D.barrier(info)
    if prof is not None:
        prof.__exit__(None, None, None)
        _export_trace(prof, cfg.log.profile_dir, info.rank)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    secs = time.time() - t0
    if cfg.dist.check_sync_every:
        check_sync(engine, info)
    if ckpt_path:
        if info.rank == 0:
            save_mlp_checkpoint(ckpt_path, engine, cfg, sizes, steps)
        D.barrier(info)
    final = hist[-1] if hist else {}
    sps = done * global_b / secs if secs > 0 else None
    return {"val_acc": final.get("val_acc"), "val_logloss": final.get("val_loss"), "samples_per_sec": sps,
            "world_size": info.world, "trivial_acc": final.get("val_trivial_acc"), "model": cfg.model, "engine": engine.name, "sizes": list(sizes), "world": info.world,
            "device": str(dev), "steps": steps, "start_step": start_step, "global_batch": global_b,
            "train_samples": margin, "val_samples": n_samples - margin,
            "seconds": round(secs, 3),
            "loss": final.get("loss"), "val": {k[4:]: v for k, v in final.items() if k.startswith("val_")},
            "history": hist, "checkpoint": ckpt_path}


# ---------------------------------------------------------------------------------------------
# random forest
# ---------------------------------------------------------------------------------------------
def train_rf(cfg: RunConfig) -> dict:
    from .models.forest import RandomForest, draw_features
    from .models.losses import draw_metrics_torch

    log = L.get("Trainer")
    if cfg.data.source == "device":
        return _train_rf_device(cfg, log)
    info = D.init(cfg.dist.backend, cfg.dist.timeout_s, device=cfg.rf.device if cfg.rf.device != "auto" else cfg.device)
    try:
        ds = load_draws(cfg)
        X, Y, F = draw_features(ds.numbers, cfg.data.lags)
        n = len(X)
        margin = positional_split(n, cfg.data.train_pct)
        r = cfg.rf
        dev = "cuda" if info.device.type == "cuda" else "cpu"
        t0 = time.time()
        rf = RandomForest(r.n_trees, r.max_depth, r.min_samples_leaf, r.feature_subset, r.bootstrap, r.seed, dev)
        rf.fit(X[:margin], Y[:margin], F, group=info.group)
        secs = time.time() - t0
        log.info(f"forest: {r.n_trees} trees depth {r.max_depth} on {margin} rows ({rf.backend_used}, "
                 f"world {info.world}) in {secs:.3f}s")
        res = {"model": "rf", "backend": rf.backend_used, "world": info.world, "trees": int(len(rf.feat)),
               "train_samples": margin, "val_samples": n - margin, "seconds": round(secs, 3)}
        if n > margin:
            p = rf.predict_proba(X[margin:])
            z = torch.logit(torch.from_numpy(p).double().clamp(1e-7, 1 - 1e-7)).float()
            yt = torch.from_numpy(multi_hot(ds.numbers[margin + cfg.data.lags:]))
            res["val"] = draw_metrics_torch(z, yt[:len(z)], "bce")
        if r.oob:  # (after the gather: every rank holds all the trees, rank 0's result is the forest's)
            res["oob"] = rf.oob_score(X[:margin], Y[:margin])
            imp = rf.feature_importances("gain")
            res["importances_top"] = [[int(f), float(imp[f])] for f in np.argsort(-imp, kind="stable")[:5]]
        if cfg.ckpt.path and info.rank == 0:
            rf.save(cfg.ckpt.path)
            res["checkpoint"] = cfg.ckpt.path
        return res
    finally:
        D.shutdown(info)


def _train_rf_device(cfg: RunConfig, log) -> dict:
    """``train --model rf --data-source device``: the draws are generated on the GPU and the packed lag-window
    rows, the fit, the validation logits, the metrics and the out-of-bag score all read device tensors
    (``ops.tree_inputs``).  Result keys as :func:`train_rf`."""
    from . import pipeline as P
    from .data.device_gen import generate_masks
    from .models.forest import RandomForest, n_candidates
    from .ops import forest as K
    from .ops import tree_inputs as TI

    r, lags = cfg.rf, int(cfg.data.lags)
    P.device_tree_guard(cfg, r.device)
    if not 1 <= lags <= TI.MAX_LAGS:
        raise ValueError(f"data.lags={lags}: the forest takes 1..{TI.MAX_LAGS} lags (at most 256 features)")
    dev = torch.device("cuda", torch.cuda.current_device())
    n_draws = P.device_draw_count(cfg)
    n = n_draws - lags
    margin = positional_split(n, cfg.data.train_pct) if n > 0 else 0
    if margin < 1:
        raise ValueError(f"need more draws than lags+1 for a training split (have {n_draws})")
    rf = RandomForest(r.n_trees, r.max_depth, r.min_samples_leaf, r.feature_subset, r.bootstrap, r.seed, "cuda")
    F, W, chunk = 62 * lags, TI.rf_words(lags), 1 << 22
    fit_bytes = K.fit_buffer_bytes(margin, W, F, r.n_trees, r.max_depth, n_candidates(r.feature_subset, F))
    oob_bytes = (8 * (W + 1) + 64 * 4 + 4) * margin if r.oob else 0  # rows, targets, out, count
    val_bytes = (8 * (W + 1) + 64 * 4) * min(chunk, n - margin)
    P.check_device_memory(8 * n_draws + max(fit_bytes, oob_bytes, val_bytes), dev, "rf on data.source=device")
    masks = generate_masks(n_draws, seed=cfg.data.seed, planted=cfg.data.planted, device=dev)
    t0 = time.time()
    rf.fit_draw_masks(masks, lags, rows=(0, margin))
    secs = time.time() - t0
    log.info(f"forest: {r.n_trees} trees depth {r.max_depth} on {margin} rows of {n_draws} device draws "
             f"({rf.backend_used}) in {secs:.3f}s")
    res = {"model": "rf", "backend": rf.backend_used, "world": 1, "trees": int(len(rf.feat)),
           "train_samples": margin, "val_samples": n - margin, "seconds": round(secs, 3)}
    if n > margin:
        def logits_of(c0, c1):
            return rf.predict_proba_device(TI.rf_rows(masks, lags, first=c0, count=c1 - c0)[0], out_logit=True)

        res["val"] = P.device_draw_metrics(masks, logits_of, margin, n, lags=lags, loss="bce", chunk=chunk)
    if r.oob:
        X, Y, _ = TI.rf_rows(masks, lags, first=0, count=margin)  # the rows of the fit, in its order
        out, count = K.oob_predict(X, rf.feat, rf.value, rf.max_depth, rf.seed, rf.tree_start)
        res["oob"] = K.oob_metrics(out, count, Y)
        imp = rf.feature_importances("gain")
        res["importances_top"] = [[int(f), float(imp[f])] for f in np.argsort(-imp, kind="stable")[:5]]
    if cfg.ckpt.path:
        rf.save(cfg.ckpt.path)
        res["checkpoint"] = cfg.ckpt.path
    return res


# ---------------------------------------------------------------------------------------------
# transition-count baseline
# ---------------------------------------------------------------------------------------------
def train_counts(cfg: RunConfig) -> dict:
    """``train --model counts``: fit the count table on the positional training split, report ``val`` on the rest.
    On a GPU the counts and the validation logits come from ``csrc/draw_counts.hip``; with ``--device cpu`` (or no
    GPU) from the numpy specification, which gives the same table."""
    from .data.draws import mask_bits
    from .models.count_table import CountTable

    log = L.get("Trainer")
    if cfg.data.source == "device":
        return _train_counts_device(cfg, log)
    lags = int(cfg.data.lags)
    ds = load_draws(cfg)
    n = len(ds) - lags
    margin = positional_split(n, cfg.data.train_pct) if n > 0 else 0
    if margin < 1:
        raise ValueError(f"need more draws than lags+1 for a training split (have {len(ds)})")
    model = CountTable(lags, cfg.counts.alpha, cfg.device)
    t0 = time.time()
    if model._use_gpu():
        from .models.mlp import FusedSmallMLP

        masks = FusedSmallMLP.prepare(ds.numbers)
        model.fit_draw_masks(masks, 0, margin)
        val = model.evaluate(masks, n - margin, offset=margin) if n > margin else None
    else:
        masks = mask_bits(ds.numbers)
        model.fit_masks_np(masks, 0, margin)
        val = model.evaluate_np(masks, margin, n - margin) if n > margin else None
    secs = time.time() - t0
    log.info(f"count table: {lags} lag(s), alpha {model.alpha:g} on {margin} samples ({model.backend_used}) in {secs:.3f}s")
    return _counts_result(cfg, model, margin, n - margin, secs, val)


def _counts_result(cfg: RunConfig, model, train_samples: int, val_samples: int, secs: float, val) -> dict:
    res = {"model": "counts", "backend": model.backend_used, "lags": model.lags, "alpha": model.alpha,
           "train_samples": int(train_samples), "val_samples": int(val_samples), "seconds": round(secs, 3),
           "val": val, "checkpoint": None}
    if cfg.ckpt.path:
        model.save(cfg.ckpt.path)
        res["checkpoint"] = cfg.ckpt.path
    return res


def _train_counts_device(cfg: RunConfig, log) -> dict:
    """``train --model counts --data-source device``: the draws are generated on the GPU and the counts, the
    validation logits and the metrics all read device tensors.  Result keys as :func:`train_counts`."""
    from . import pipeline as P
    from .data.device_gen import generate_masks
    from .models.count_table import CountTable

    lags = int(cfg.data.lags)
    P.device_tree_guard(cfg, "auto")
    dev = torch.device("cuda", torch.cuda.current_device())
    n_draws = P.device_draw_count(cfg)
    n = n_draws - lags
    margin = positional_split(n, cfg.data.train_pct) if n > 0 else 0
    if margin < 1:
        raise ValueError(f"need more draws than lags+1 for a training split (have {n_draws})")
    chunk = 1 << 22
    # the masks, one chunk of validation logits, and the counts' and metrics' small buffers
    P.check_device_memory(8 * n_draws + 64 * 4 * min(chunk, max(n - margin, 1)) + (1 << 22), dev,
                          "counts on data.source=device")
    masks = generate_masks(n_draws, seed=cfg.data.seed, planted=cfg.data.planted, device=dev)
    model = CountTable(lags, cfg.counts.alpha, "cuda")
    t0 = time.time()
    model.fit_draw_masks(masks, 0, margin)
    secs = time.time() - t0
    log.info(f"count table: {lags} lag(s), alpha {model.alpha:g} on {margin} samples of {n_draws} device draws "
             f"({model.backend_used}) in {secs:.3f}s")
    val = None
    if n > margin:
        val = P.device_draw_metrics(masks, lambda c0, c1: model.logits(masks, c1 - c0, offset=c0), margin, n,
                                    lags=lags, loss="softmax", chunk=chunk)
    return _counts_result(cfg, model, margin, n - margin, secs, val)


# ---------------------------------------------------------------------------------------------
def train(cfg: RunConfig) -> dict:
    if cfg.model in ("mlp", "mlp-wide"):
        return train_mlp(cfg)
    if cfg.model == "rf":
        return train_rf(cfg)
    if cfg.model == "counts":
        return train_counts(cfg)
    if cfg.model == "gbdt":
        return run_reference_pipeline(cfg)
    raise ValueError(f"unknown model {cfg.model!r}")


def _top_pick(p: np.ndarray) -> tuple[list[int], list[int]]:
    main = sorted(int(i) + 1 for i in np.argsort(-p[:50], kind="stable")[:5])
    stars = sorted(int(i) + 1 for i in np.argsort(-p[50:62], kind="stable")[:2])
    return main, stars


def predict_next(cfg: RunConfig) -> dict:
    """Predict the draw after the last one in the configured data from a checkpoint."""
    path = cfg.ckpt.resume or cfg.ckpt.path
    if not path:
        raise ValueError("predict needs --ckpt (or --resume) pointing at a checkpoint")
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    ds = load_draws(cfg)
    if path.endswith(".npz"):
        from .models.forest import RandomForest, draw_features, pack_bits

        rf = RandomForest.load(path)
        lags = rf.F // 62
        x = pack_bits(multi_hot(ds.numbers[len(ds) - lags:]).reshape(1, -1))
        p = rf.predict_proba(x)[0]
        kind = "rf"
    elif path.endswith(".json"):
        from .models.gbdt import GBDT

        g = GBDT.load(path)
        x = multi_hot(ds.numbers[-1:]).astype(np.float64)
        nf = len(g.cuts) if g.cuts is not None else (g.num_feature or 62)
        if nf > 62 and ds.dates is not None:
            from .data.draws import featurize_raw

            x = np.concatenate([x, featurize_raw(ds)[-1:, :4].astype(np.float64)], axis=1)
        p = np.asarray(g.predict(x))[0]
        kind = "gbdt"
    elif path.endswith(".cnt"):
        from .data.draws import mask_bits
        from .models.count_table import CountTable

        ct = CountTable.load(path, "cpu")
        if len(ds) < ct.lags:
            raise ValueError(f"the checkpoint reads {ct.lags} draws, the data gives {len(ds)}")
        # one row through the numpy specification: the sample whose window is the last `lags` draws
        z = ct.logits_np(mask_bits(ds.numbers), [len(ds) - ct.lags])[0, :62].astype(np.float64)
        e = np.exp(z - np.concatenate([np.full(50, z[:50].max()), np.full(12, z[50:].max())]))
        p = np.concatenate([e[:50] / e[:50].sum(), e[50:] / e[50:].sum()])
        kind = "counts"
    else:
        from .models import losses as LS
        from .models.mlp import DrawMLP

        ck = load_mlp_checkpoint(path)
        sizes = ck["sizes"]
        ex = ck["extra"]
        lags = int(ex.get("lags", sizes[0] // 62))
        net = DrawMLP(sizes, activation=ex.get("activation", "relu"), loss=ex.get("loss", "softmax"), use_hip=False)
        net.load_state_dict(ck["state_dict"])
        x = torch.from_numpy(multi_hot(ds.numbers[len(ds) - lags:]).reshape(1, -1))
        with torch.no_grad():
            z = net(x)[0]
        if ex.get("loss", "softmax") == "softmax":
            p = torch.cat([torch.softmax(z[LS.MAIN], 0), torch.softmax(z[LS.STAR], 0)]).numpy()
        else:
            p = torch.sigmoid(z).numpy()
        kind = "mlp"
    main, stars = _top_pick(np.asarray(p, dtype=np.float64))
    nxt = next_draw_date(ds.dates[-1]) if ds.dates is not None and len(ds.dates) else None
    res = {"model": kind, "checkpoint": path, "after_draw": date_str(ds.dates[-1]) if ds.dates is not None else None,
           "next_draw_date": date_str(nxt) if nxt is not None else None, "main": main, "stars": stars,
           "p_main": [round(float(p[i - 1]), 5) for i in main], "p_stars": [round(float(p[49 + s]), 5) for s in stars]}
    print(" ".join(f"{v:02d}" for v in main) + "  *  " + " ".join(f"{v:02d}" for v in stars))
    tc = cfg.tickets
    if tc.n > 0:
        # through the numpy specification (one row): CPU and GPU boxes print the same tickets.  Scores: an
        # MLP's or the count table's logits (under bce the sampling weights are the odds), log p for the tree models
        from . import tickets as TK

        score = z.numpy().astype(np.float64) if kind == "mlp" else z if kind == "counts" else TK.log_scores(p)
        tks, _ = TK.sample_tickets_py(score[None, :62], [len(ds) - 1], tc.n, tc.temperature, tc.seed)
        res["tickets"] = []
        for t in tks[0]:
            tm, ts = TK.ticket_numbers(t)
            res["tickets"].append({"main": tm, "stars": ts})
            print(" ".join(f"{v:02d}" for v in tm) + "  *  " + " ".join(f"{v:02d}" for v in ts))
        res["ticket_sampling"] = {"n": tc.n, "temperature": tc.temperature, "seed": tc.seed}
    return res


def gbdt_feature_names(n_features: int) -> list[str]:
    """Names of the next-draw GBDT's input columns: the 50 numbers and 12 stars of the last draw, then its date
    fields (``pipeline.gbdt_dataset``)."""
    names = [f"number {i + 1}" for i in range(50)] + [f"star {i + 1}" for i in range(12)]
    names += ["weekday", "month", "day", "year"]
    return (names + [f"f{i}" for i in range(len(names), n_features)])[:n_features]


def explain_next(cfg: RunConfig, top: int = 3) -> dict:
    """``euromillioner explain``: for each number and star a GBDT (.json) or forest (.npz) checkpoint picks for the
    next draw, the ``top`` features with the largest |TreeSHAP contribution| to that pick's margin (GBDT) or
    probability (forest)."""
    path = cfg.ckpt.resume or cfg.ckpt.path
    if not path:
        raise ValueError("explain needs --ckpt (or --resume) pointing at a GBDT or forest checkpoint")
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    if not path.endswith((".json", ".npz")):
        raise ValueError(f"explain covers GBDT (.json) and forest (.npz) checkpoints only, not {os.path.basename(path)}")
    if top < 1:
        raise ValueError("--top must be at least 1")
    if path.endswith(".npz"):
        return _explain_forest(cfg, path, top)
    from .models.gbdt import GBDT
    from .models.gbdt_explain import num_features
    from .pipeline import _gbdt_backend

    ds = load_draws(cfg)
    g = GBDT.load(path)
    if g.n_tasks != 62:
        raise ValueError(f"explain needs a next-draw GBDT (62 boosters), this checkpoint has {g.n_tasks}")
    nf = num_features(g)
    x = multi_hot(ds.numbers[-1:]).astype(np.float64)
    if nf > 62 and ds.dates is not None:
        from .data.draws import featurize_raw

        x = np.concatenate([x, featurize_raw(ds)[-1:, :4].astype(np.float64)], axis=1)
    if x.shape[1] != nf:
        raise ValueError(f"the checkpoint expects {nf} features, the data gives {x.shape[1]}")
    be = g._explain_backend(_gbdt_backend(cfg))
    phi = np.asarray(g.predict_contribs(x, backend=be), dtype=np.float64)[0]  # [62, F+1]
    main, stars = _top_pick(phi.sum(axis=1))  # sum == margin; the logistic transform keeps the order
    names = gbdt_feature_names(nf)
    picks = []
    for kind, v, t in [("number", v, v - 1) for v in main] + [("star", v, 49 + v) for v in stars]:
        order = np.argsort(-np.abs(phi[t, :nf]), kind="stable")[:top]
        feats = [{"feature": names[f], "index": int(f), "phi": round(float(phi[t, f]), 6)} for f in order]
        picks.append({"pick": f"{kind} {v}", "margin": round(float(phi[t].sum()), 6), "bias": round(float(phi[t, nf]), 6),
                      "top": feats})
        print(f"{kind} {v:02d}: " + ", ".join(f"{d['feature']} {d['phi']:+.4f}" for d in feats))
    return {"model": "gbdt", "checkpoint": path, "backend": be, "main": main, "stars": stars,
            "after_draw": date_str(ds.dates[-1]) if ds.dates is not None else None, "explain": picks}


def _explain_forest(cfg: RunConfig, path: str, top: int) -> dict:
    """The forest half of :func:`explain_next`: the input row is the last ``lags = F / 62`` draws, the picks are
    the largest ``predict_proba`` entries (== ``phi.sum``), the features are named after ``lag_features``."""
    from .models.forest import RandomForest, pack_bits
    from .models.forest_explain import feature_names

    ds = load_draws(cfg)
    rf = RandomForest.load(path)
    F = int(rf.F)
    lags = F // 62
    if lags < 1 or F != 62 * lags:
        raise ValueError(f"explain needs a next-draw forest over 62 features per draw, this checkpoint has {F}")
    if len(ds) < lags:
        raise ValueError(f"the checkpoint expects {F} features ({lags} draws), the data gives {62 * len(ds)}")
    x = pack_bits(multi_hot(ds.numbers[len(ds) - lags:]).reshape(1, -1))
    # --device cpu: the numpy path; otherwise the device when there is one and the forest is inside its plan
    phi = rf.predict_contribs(x, backend="numpy" if cfg.device == "cpu" else None)
    phi, be = np.asarray(phi, dtype=np.float64)[0], rf.explain_backend_used  # [62, F+1]
    main, stars = _top_pick(phi.sum(axis=1))  # sum == predict_proba
    names = feature_names(F)
    picks = []
    for kind, v, t in [("number", v, v - 1) for v in main] + [("star", v, 49 + v) for v in stars]:
        order = np.argsort(-np.abs(phi[t, :F]), kind="stable")[:top]
        feats = [{"feature": names[f], "index": int(f), "phi": round(float(phi[t, f]), 6)} for f in order]
        picks.append({"pick": f"{kind} {v}", "proba": round(float(phi[t].sum()), 6), "bias": round(float(phi[t, F]), 6),
                      "top": feats})
        print(f"{kind} {v:02d}: " + ", ".join(f"{d['feature']} {d['phi']:+.4f}" for d in feats))
    return {"model": "rf", "checkpoint": path, "backend": be, "main": main, "stars": stars,
            "after_draw": date_str(ds.dates[-1]) if ds.dates is not None else None, "explain": picks}


def _backtest_numpy(net, ds, lags: int, margin: int, n_samples: int, tc, chunk: int = 1 << 14):
    """DrawMLP logits + the numpy specification (the --device cpu path; row id = sample index, as on the GPU)."""
    from . import tickets as TK
    from .data.draws import mask_bits

    X, _ = lag_features(ds.numbers, lags)
    targets = mask_bits(ds.numbers)[lags:]  # sample i is scored against draw i + lags
    hist, best = np.zeros((6, 3), dtype=np.int64), np.zeros(14, dtype=np.int64)
    for a in range(margin, n_samples, chunk):
        b = min(a + chunk, n_samples)
        with torch.no_grad():
            z = net(torch.from_numpy(X[a:b])).numpy()
        tks, _ = TK.sample_tickets_py(z, np.arange(a, b), tc.n, tc.temperature, tc.seed)
        h, bt = TK.score_tickets_py(tks, targets[a:b])
        hist += h
        best += bt
    return hist, best


def backtest(cfg: RunConfig) -> dict:
    """``euromillioner backtest``: play ``tickets.n`` sampled tickets on every draw of the positional validation
    split and count prize tiers, next to the expectation of uniformly random play.  MLP checkpoints and count tables (``.cnt``, :func:`_backtest_counts`); for an MLP on a
    GPU the logits and the tickets never leave the device (csrc/tickets.hip), on ``--device cpu`` the same
    numbers come from DrawMLP and the numpy specification."""
    from .models.mlp import DrawMLP
    from .ops.tickets import backtest_result

    path = cfg.ckpt.resume or cfg.ckpt.path
    if not path:
        raise ValueError("backtest needs --ckpt pointing at an MLP checkpoint")
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    if path.endswith((".npz", ".json")):
        raise ValueError("backtest covers MLP checkpoints (predict --tickets samples from RF / GBDT models)")
    tc = cfg.tickets
    if tc.n < 1:
        raise ValueError("backtest needs --tickets N with N in 1..64")
    if path.endswith(".cnt"):
        return _backtest_counts(cfg, path)
    ck = load_mlp_checkpoint(path)
    sizes, ex = tuple(ck["sizes"]), ck["extra"]
    lags = int(ex.get("lags", sizes[0] // 62))
    act, loss = ex.get("activation", "relu"), ex.get("loss", "softmax")
    ds = load_draws(cfg)
    n_samples = len(ds) - lags
    margin = positional_split(n_samples, cfg.data.train_pct)
    rows = n_samples - margin
    if rows < 1:
        raise ValueError("empty validation split")
    use_gpu = cfg.device == "cuda" or (cfg.device == "auto" and torch.cuda.is_available())
    if use_gpu:
        from .models.mlp import FusedSmallMLP

        if sizes == (62, 128, 62) and act == "relu":
            model = FusedSmallMLP("cuda", loss=loss, dtype=cfg.mlp.dtype,
                                  state_dict={_FusedEngine._MAP[k]: v for k, v in ck["state_dict"].items()})
        else:
            from .models.gemm_mlp import GemmMLPTrainer

            model = GemmMLPTrainer(sizes, "cuda", activation=act, loss=loss, state_dict=ck["state_dict"],
                                   dtype=cfg.mlp.dtype, lags=lags)
        masks = FusedSmallMLP.prepare(torch.from_numpy(ds.numbers).cuda())
        r = model.backtest(masks, rows, tc.n, tc.temperature, tc.seed, offset=margin)
        engine = "hip"
    else:
        net = DrawMLP(sizes, activation=act, loss=loss, use_hip=False)
        net.load_state_dict(ck["state_dict"])
        r = backtest_result(*_backtest_numpy(net, ds, lags, margin, n_samples, tc), rows, tc.n)
        engine = "numpy"
    return _backtest_report({"model": "mlp", "checkpoint": path, "engine": engine, "sizes": list(sizes)}, r, rows, tc)


def _backtest_counts(cfg: RunConfig, path: str) -> dict:
    """The count-table half of :func:`backtest` (a ``.cnt`` checkpoint): ``CountTable.backtest`` on a GPU, the numpy
    specification plus ``sample_tickets_py`` / ``score_tickets_py`` on ``--device cpu``."""
    from . import tickets as TK
    from .data.draws import mask_bits
    from .models.count_table import CountTable
    from .ops.tickets import backtest_result

    tc = cfg.tickets
    use_gpu = cfg.device == "cuda" or (cfg.device == "auto" and torch.cuda.is_available())
    ct = CountTable.load(path, "cuda" if use_gpu else "cpu")
    ds = load_draws(cfg)
    n_samples = len(ds) - ct.lags
    margin = positional_split(n_samples, cfg.data.train_pct)
    rows = n_samples - margin
    if rows < 1:
        raise ValueError("empty validation split")
    if use_gpu:
        from .models.mlp import FusedSmallMLP

        masks = FusedSmallMLP.prepare(ds.numbers)
        r = ct.backtest(masks, rows, tc.n, tc.temperature, tc.seed, offset=margin)
        engine = "hip"
    else:
        masks = mask_bits(ds.numbers)
        hist, best = np.zeros((6, 3), dtype=np.int64), np.zeros(14, dtype=np.int64)
        for a in range(margin, n_samples, 1 << 14):  # (row id = sample index, as on the GPU)
            b = min(a + (1 << 14), n_samples)
            idx = np.arange(a, b)
            tks, _ = TK.sample_tickets_py(ct.logits_np(masks, idx), idx, tc.n, tc.temperature, tc.seed)
            h, bt = TK.score_tickets_py(tks, masks[a + ct.lags:b + ct.lags])
            hist += h
            best += bt
        r = backtest_result(hist, best, rows, tc.n)
        engine = "numpy"
    return _backtest_report({"model": "counts", "checkpoint": path, "engine": engine, "lags": ct.lags}, r, rows, tc)


def _backtest_report(head: dict, r: dict, rows: int, tc) -> dict:
    """Print the prize-tier table of a back-test and return its result (``head`` first)."""
    from . import tickets as TK

    tiers, exp_t = TK.tier_counts(r["hist"]), r["uniform"]["tiers"]
    print(f"{rows} draws x {tc.n} tickets (T={tc.temperature:g}, seed {tc.seed}): tickets per prize tier | "
          f"draws by best ticket (uniform play beside each)")
    for k in range(13):
        print(f"{k + 1:>2} {TK.TIER_NAMES[k]:>4} {int(tiers[k]):>12} {exp_t[k]:>14.3f} | "
              f"{int(r['best'][k]):>12} {r['uniform']['best'][k]:>14.3f}")
    return {**head, "rows": rows, "tickets": r["tickets"], "n_tickets": tc.n, "temperature": tc.temperature, "seed": tc.seed,
            "hist": r["hist"].tolist(), "best": r["best"].tolist(), "tiers": tiers.tolist(),
            "uniform": {k: np.asarray(v).tolist() for k, v in r["uniform"].items()}}


# ---------------------------------------------------------------------------------------------
# evaluate: any checkpoint on the validation split, with a calibration report
# ---------------------------------------------------------------------------------------------
def _eval_edges(cfg: RunConfig) -> tuple:
    """``eval.edges``: None (the default edges) or a comma list of probabilities."""
    from . import calibration as CAL

    e = cfg.eval.edges
    if e is None:
        return CAL.DEFAULT_EDGES
    if isinstance(e, (int, float)):
        e = (e,)
    elif isinstance(e, str):
        try:
            e = tuple(float(p) for p in e.split(",") if p.strip())
        except ValueError as err:
            raise ValueError(f"eval.edges={cfg.eval.edges!r}: a comma list of probabilities ({err})") from err
    return CAL.check_edges(e)


def _evaluate_numpy(logits_of, targets: np.ndarray, a: int, b: int, loss: str, edges, chunk: int = 1 << 14) -> dict:
    """The ``--device cpu`` engine: ``logits_of(c0, c1)`` gives the [c1 - c0, >= 62] logits of samples [c0, c1), which
    are scored against the masks ``targets[c0:c1]`` by ``metrics.draw_metrics`` and ``calibration.calibration_np``."""
    from . import calibration as CAL
    from .metrics import draw_metrics
    from .models.count_table import _bits

    keys = ("loss", "acc", "acc_thr", "hits_main", "hits_star", "exact", "trivial_acc")
    tot, totals = np.zeros(len(keys), dtype=np.float64), None
    for c0 in range(a, b, chunk):
        c1 = min(b, c0 + chunk)
        z = np.asarray(logits_of(c0, c1))[:, :62]
        tm = targets[c0:c1]
        r = draw_metrics(z.astype(np.float64), _bits(tm.view(np.uint64))[:, :62], loss)
        tot += np.array([r[k] for k in keys]) * (c1 - c0)
        totals = CAL.add_totals(totals, CAL.calibration_np(z, tm, loss, edges))
    val = {k: float(tot[i] / (b - a)) for i, k in enumerate(keys)}
    val["count"] = int(b - a)
    return {"val": val, "calibration": CAL.report(totals, b - a, loss, edges)}


class _EvalSetup(NamedTuple):
    """What scoring a checkpoint needs, whatever its kind (:func:`_eval_setup`).  On a GPU ``logits_of(b, offset,
    sidx)`` returns device logits [b, >= 64] that are scored against ``targets[idx + 1]`` (device masks), in chunks of
    ``chunk``; on the host ``logits_of(c0, c1)`` returns the logits of samples [c0, c1), scored against the host
    masks ``targets[c0:c1]``."""
    path: str
    head: dict
    edges: tuple
    use_gpu: bool
    loss: str
    lags: int
    margin: int
    n: int
    logits_of: Any
    targets: Any
    chunk: int


def _eval_setup(cfg: RunConfig, model: str | None, what: str) -> _EvalSetup:
    """The per-kind set-up of ``evaluate`` and ``calibrate``: the checkpoint kind (read from the file; ``model``, the
    CLI's ``--model``, must agree with it when given), its logits, the target masks, the loss, the validation
    samples ``[margin, n)`` and the head of the result."""
    from .data.draws import mask_bits

    path = cfg.ckpt.resume or cfg.ckpt.path
    if not path:
        raise ValueError(f"{what} needs --ckpt pointing at a checkpoint")
    if not os.path.exists(path):
        raise FileNotFoundError(path)
    kind = {".npz": "rf", ".json": "gbdt", ".cnt": "counts"}.get(os.path.splitext(path)[1], "mlp")
    if model is not None and {"mlp-wide": "mlp"}.get(model, model) != kind:
        raise ValueError(f"--model {model} was asked for, {os.path.basename(path)} is a {kind} checkpoint")
    edges = _eval_edges(cfg)
    use_gpu = cfg.device == "cuda" or (cfg.device == "auto" and torch.cuda.is_available())
    ds = load_draws(cfg)
    host_masks = mask_bits(ds.numbers).view(np.int64)
    head: dict = {"checkpoint": path, "engine": "hip" if use_gpu else "numpy"}
    chunk = 1 << 20

    def split(lags: int) -> tuple[int, int]:
        n = len(ds) - lags
        margin = positional_split(n, cfg.data.train_pct) if n > 0 else 0
        if n - margin < 1:
            raise ValueError("empty validation split")
        return margin, n

    def device_masks():
        from .models.mlp import FusedSmallMLP

        return FusedSmallMLP.prepare(ds.numbers)

    if path.endswith(".npz"):
        from .models.forest import RandomForest, pack_bits

        rf = RandomForest.load(path)
        lags = int(rf.F) // 62
        if lags < 1 or int(rf.F) != 62 * lags:
            raise ValueError(f"{what} needs a next-draw forest over 62 features per draw, this checkpoint has {rf.F}")
        margin, n = split(lags)
        loss = "bce"
        head.update(model="rf", lags=lags, trees=int(len(rf.feat)))
        if use_gpu:
            from .ops import tree_inputs as TI

            masks = device_masks()
            targets = masks[lags - 1:] if lags > 1 else masks  # as pipeline.device_draw_metrics

            def logits_of(b, o, si):
                return rf.predict_proba_device(TI.rf_rows(masks, lags, first=o, count=b)[0], out_logit=True)
        else:
            X, _ = lag_features(ds.numbers, lags)
            targets = host_masks[lags:]

            def logits_of(c0, c1):
                p = rf.predict_proba(pack_bits(X[c0:c1]))
                return torch.logit(torch.from_numpy(p).double().clamp(1e-7, 1 - 1e-7)).float().numpy()  # as train_rf
    elif path.endswith(".json"):
        from .data.draws import featurize_raw
        from .models.gbdt import GBDT
        from .models.gbdt_explain import num_features

        g = GBDT.load(path)
        if g.n_tasks != 62 or g.objective not in ("reg:logistic", "binary:logistic"):
            raise ValueError(f"{what} needs a 62-booster logistic next-draw GBDT; this checkpoint has {g.n_tasks} "
                             f"booster(s) with objective {g.objective}")
        nf = num_features(g)
        lags = 1
        margin, n = split(1)
        loss = "bce"
        head.update(model="gbdt", features=nf)

        def host_margin(c0, c1):
            x = multi_hot(ds.numbers[c0:c1]).astype(np.float64)
            if nf > 62 and ds.dates is not None:
                x = np.concatenate([x, featurize_raw(ds)[c0:c1, :4].astype(np.float64)], axis=1)
            if x.shape[1] != nf:
                raise ValueError(f"the checkpoint expects {nf} features, the data gives {x.shape[1]}")
            return g.predict_margin(x)

        if use_gpu:
            targets = masks = device_masks()
            if nf == 62:
                def logits_of(b, o, si):
                    return g.predict_margin_draw_masks(masks, (o, o + b))
            else:  # date columns: the margins of the host rows, uploaded as [rows, 64]
                def logits_of(b, o, si):
                    z = torch.zeros(b, 64, dtype=torch.float32)
                    z[:, :62] = torch.from_numpy(np.asarray(host_margin(o, o + b), dtype=np.float32))
                    return z.cuda()
        else:
            logits_of, targets = host_margin, host_masks[1:]
    elif path.endswith(".cnt"):
        from .models.count_table import CountTable

        ct = CountTable.load(path, "cuda" if use_gpu else "cpu")
        lags = ct.lags
        margin, n = split(ct.lags)
        loss = "softmax"
        head.update(model="counts", lags=ct.lags)
        if use_gpu:
            masks = device_masks()
            targets = ct._tmasks(masks)

            def logits_of(b, o, si):
                return ct.logits(masks, b, offset=o, sidx=si)
        else:
            targets = host_masks[ct.lags:]

            def logits_of(c0, c1):
                return ct.logits_np(host_masks, np.arange(c0, c1))
    else:
        from .models.mlp import DrawMLP

        ck = load_mlp_checkpoint(path)
        sizes, ex = tuple(ck["sizes"]), ck["extra"]
        lags = int(ex.get("lags", sizes[0] // 62))
        act, loss = ex.get("activation", "relu"), ex.get("loss", "softmax")
        margin, n = split(lags)
        head.update(model="mlp", sizes=list(sizes), lags=lags)
        if use_gpu:
            from .models.mlp import FusedSmallMLP

            masks = device_masks()
            chunk = 1 << 16
            if sizes == (62, 128, 62) and act == "relu":
                net = FusedSmallMLP("cuda", loss=loss, dtype=cfg.mlp.dtype,
                                    state_dict={_FusedEngine._MAP[k]: v for k, v in ck["state_dict"].items()})
                targets = masks
            else:
                from .models.gemm_mlp import GemmMLPTrainer

                net = GemmMLPTrainer(sizes, "cuda", activation=act, loss=loss, state_dict=ck["state_dict"],
                                     dtype=cfg.mlp.dtype, lags=lags)
                targets = net._tmasks(masks)

            def logits_of(b, o, si):
                return net.logits(masks, b, offset=o, sidx=si)
        else:
            net = DrawMLP(sizes, activation=act, loss=loss, use_hip=False)
            net.load_state_dict(ck["state_dict"])
            X, _ = lag_features(ds.numbers, lags)
            targets = host_masks[lags:]

            def logits_of(c0, c1):
                with torch.no_grad():
                    return net(torch.from_numpy(X[c0:c1])).numpy()
    return _EvalSetup(path, head, edges, use_gpu, loss, int(lags), margin, n, logits_of, targets, chunk)


def _score(s: _EvalSetup, first: int, cal=None) -> dict:
    """``{"val", "calibration"}`` of the samples ``[first, n)`` of a set-up, through the calibrator ``cal`` if given."""
    if s.use_gpu:
        from .ops import calibration as OC

        logits_of = s.logits_of
        if cal is not None:
            from .ops import calibration_fit as CF

            def logits_of(b, o, si):
                return CF.apply_scaling(s.logits_of(b, o, si), b, cal.a, cal.b)

        return OC.calibrate_logits(logits_of, s.targets, s.n - first, s.loss, s.edges, offset=first, chunk=s.chunk)
    logits_of = s.logits_of if cal is None else (lambda c0, c1: cal.apply_np(s.logits_of(c0, c1)))
    return _evaluate_numpy(logits_of, s.targets, first, s.n, s.loss, s.edges)


def _check_calibrator(cal, s: _EvalSetup, path: str) -> None:
    """A calibrator is for one checkpoint kind, head and lag count, and must leave samples to score."""
    rec = cal.record
    if rec.get("model") != s.head["model"] or cal.loss != s.loss or rec.get("lags") != s.lags:
        raise ValueError(f"{os.path.basename(path)} was fitted for a {rec.get('model')} checkpoint ({cal.loss} head, "
                         f"lags {rec.get('lags')}); this one is {s.head['model']} ({s.loss} head, lags {s.lags})")
    last = rec.get("last")
    if not isinstance(last, int) or not s.margin <= last < s.n:
        raise ValueError(f"{os.path.basename(path)} was fitted on samples up to {last}: no validation sample of "
                         f"[{s.margin}, {s.n}) is left to score")


def evaluate(cfg: RunConfig, model: str | None = None) -> dict:
    """``euromillioner evaluate``: score a checkpoint of any of the five model kinds on the positional validation
    split (the kind is read from the checkpoint; ``model``, the CLI's ``--model``, must agree with it when given): the draw metrics of ``train`` plus a calibration report (reliability table per group, Brier score,
    expected calibration error; :mod:`euromillioner_amd.calibration`).  On a GPU the logits stay on the device
    (``ops.calibration``); ``--device cpu`` runs the numpy specification on the model's host logits.

    With ``eval.calibrator`` (``--calibrator F``, a ``.cal`` file of ``calibrate``) the samples after the calibrator's
    fit range, ``[cal.last, n)``, are scored through it."""
    from . import calibration as CAL

    s = _eval_setup(cfg, model, "evaluate")
    cal, first, note, extra = None, s.margin, "", {}
    if cfg.eval.calibrator is not None:
        from .scaling import Calibrator

        cpath = str(cfg.eval.calibrator)
        if not os.path.exists(cpath):
            raise FileNotFoundError(cpath)
        cal = Calibrator.load(cpath)
        _check_calibrator(cal, s, cpath)
        first = int(cal.record["last"])
        note = f", samples [{first}, {s.n}) through {os.path.basename(cpath)}"
        extra = {"first": first, "calibrator": cal.to_dict()}
    res = _score(s, first, cal)
    rep = res["calibration"]
    print(f"{s.n - first} validation rows, {s.head['model']} ({s.loss} head, {s.head['engine']}){note}")
    print(CAL.format_report(rep, s.edges))
    return {**s.head, "loss": s.loss, "rows": s.n - first, "val": res["val"], "calibration": rep,
            "edges": list(s.edges), **extra}


# ---------------------------------------------------------------------------------------------
# calibrate: fit a per-group scaling of a checkpoint's logits on held-out rows
# ---------------------------------------------------------------------------------------------
def calibrate(cfg: RunConfig, model: str | None = None) -> dict:
    """``euromillioner calibrate``: fit the per-group scale (and, under the sigmoid head, shift) of a checkpoint's
    logits (:mod:`euromillioner_amd.scaling`) on the first ``floor(eval.fit_pct (n - margin))`` validation samples,
    at most ``eval.fit_rows`` of them, score the remaining ones raw and calibrated, and write the ``.cal`` file to
    ``eval.out`` (default ``<ckpt>.cal``).  On a GPU the fit rows' logits fill one device buffer and every Newton
    pass is one kernel launch over it (``ops.calibration_fit``); ``--device cpu`` runs the numpy specification.
    Single process.  Returns ``{"before", "after"`` (each the ``val`` and ``calibration`` of ``evaluate``),
    ``"calibrator"}`` next to the head of ``evaluate``."""
    from . import calibration as CAL
    from . import scaling as SC

    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise ValueError("calibrate runs in a single process (no --dp, no torchrun)")
    fit_pct, fit_rows = float(cfg.eval.fit_pct), int(cfg.eval.fit_rows)
    if not 0.0 < fit_pct < 1.0:
        raise ValueError(f"eval.fit_pct={cfg.eval.fit_pct!r}: a share inside (0, 1)")
    if fit_rows < 1:
        raise ValueError(f"eval.fit_rows={cfg.eval.fit_rows!r}: at least 1")
    s = _eval_setup(cfg, model, "calibrate")
    rows = min(int(math.floor(fit_pct * (s.n - s.margin))), fit_rows)
    last = s.margin + rows
    if rows < 1 or last >= s.n:
        raise ValueError(f"{s.n - s.margin} validation samples at fit_pct {fit_pct} leave the fit or the scoring "
                         "without rows")
    if s.use_gpu:
        from .ops import calibration_fit as CF

        buf, done = torch.empty(rows, 64, dtype=torch.float32, device="cuda"), 0
        while done < rows:
            b = min(s.chunk, rows - done)
            buf[done:done + b] = s.logits_of(b, s.margin + done, None)[:, :64]
            done += b
        fit = CF.fit_device(buf, s.targets, rows, s.loss, offset=s.margin)
        del buf
    else:
        z = np.concatenate([np.asarray(s.logits_of(c0, min(last, c0 + (1 << 14))), dtype=np.float32)[:, :62]
                            for c0 in range(s.margin, last, 1 << 14)])
        fit = SC.fit_np(z, s.targets[s.margin:last], s.loss)
    cal = SC.Calibrator(s.loss, fit["a"], fit["b"], {
        "model": s.head["model"], "lags": s.lags, "first": s.margin, "last": last, "rows": rows,
        "iterations": [int(v) for v in fit["iterations"]], "converged": [bool(v) for v in fit["converged"]],
        "loss_before": SC.row_loss(fit["L_before"][:, None], rows, s.loss),
        "loss_after": SC.row_loss(fit["L_after"][:, None], rows, s.loss), "checkpoint": os.path.basename(s.path)})
    before, after = _score(s, last), _score(s, last, cal)
    out = str(cfg.eval.out) if cfg.eval.out is not None else s.path + ".cal"
    cal.save(out)
    print(f"fitted on samples [{s.margin}, {last}), scored on [{last}, {s.n}): {s.head['model']} ({s.loss} head, "
          f"{s.head['engine']})")
    for g, name in enumerate(CAL.GROUPS):
        print(f"{name}: a {float(cal.a[g]):.6g}  b {float(cal.b[g]):.6g}  ({fit['iterations'][g]} iterations, "
              f"{'converged' if fit['converged'][g] else 'stopped'})")
        for tag, r in (("before", before), ("after", after)):
            c = r["calibration"][name]
            print(f"  {tag:<7} ece {c['ece']:.6f}  brier/row {c['brier']:.6f}  loss {r['val']['loss']:.6f}")
    print(f"loss per fit row {cal.record['loss_before']:.6f} -> {cal.record['loss_after']:.6f}; wrote {out}")
    return {**s.head, "loss": s.loss, "rows": s.n - last, "fit_rows": rows, "before": before, "after": after,
            "calibrator": cal.to_dict(), "out": out, "edges": list(s.edges)}
