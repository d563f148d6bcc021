"""Horizontal-FL round around the secure aggregator (SURVEY.md §8f row 1,
BASELINE config 4): the caller side of the hot path, mirrored from the
reference so the aggregator can be swapped in exactly where FLModel uses it.

Reference interfaces followed:

* ``FLModel.fit`` aggregation hooks -- the initial weights of every worker
  are averaged through the aggregator and installed everywhere before the
  first epoch (``fl_model.py:473`` -> ``initialize_weights``, ``:126-138``);
  every ``aggregate_freq`` local steps the
  clients' ``train_step`` outputs go to ``aggregator.average(params, axis=0,
  weights=sample_nums)`` and the result is sent back to every party
  (``sfl/ml/nn/fl/fl_model.py:492-517``, ``:578-583``); the last batch of an
  epoch is applied with ``apply_weights`` (``:585-589``);
* ``FedAvgW.train_step`` -- set the global weights, run ``train_steps``
  batches, return ``(get_weights(return_numpy=True), num_sample)``
  (``sfl/ml/nn/fl/backend/torch/strategy/fed_avg_w.py:36-87``);
* torch payload packing -- ``state_dict`` values as a list of host numpy
  arrays, written back with ``torch.Tensor(np.copy(v))``
  (``sfl/ml/nn/core/torch/mixins.py:74-89``);
* ``TorchModel(model_fn, loss_fn, optim_fn, metrics)`` and ``optim_wrapper``
  (``sfl/ml/nn/core/torch/module.py:247``, ``sfl/ml/nn/core/torch/utils.py:23``);
  each worker seeds torch with ``random_seed`` before building its model
  (``sfl/ml/nn/fl/backend/torch/fl_base.py:51-52``), so every client starts
  from the same initial weights.

Parties are ``PYU``s (``sfl_amd.device``); local training runs on
``train_device`` (the party's GPU by default, or the CPU).  Out of scope:
the reference's dataset builders, callbacks, DP accountant hooks and the
other strategies (fed_prox, scaffold, ...); ``fed_smp`` (sparsified model
perturbation, ``examples/security/h_gia/FedSMP_defense/FedSMP_torch.py``) is
mirrored at the end of this text;
``moon`` is mirrored because its reference test is the FL end-to-end the
survey names for the aggregator swap, ``fed_avg_u``
and ``fed_avg_g`` because they are the other payload producers of §8(a8)
(model updates and gradients instead of weights), and ``fed_stc`` (sparse
ternary compression up- and downstream, ``fed_stc.py:42-143`` on the
workers, ``fl_model.py:542-556`` / ``compress.py:28-42`` on the server)
because it is the reference's bandwidth-reducing strategy: its per-element
work runs in the HIP kernels of ``sfl_amd.utils.compressor`` wherever
``compress_device`` is a GPU.  By default the ternary tensors travel dense:
the secure aggregator masks every element and has no sparse input.
``sparse_transport`` ("down" or "both") puts them into COO form
(``sfl_amd.utils.sparse``: on the host for host payloads, by the ``sa_coo``
kernels for a GPU model's, which then never take the dense form on the host)
as the reference's ``sparse_encode`` does at the
end of ``train_step`` (``fed_stc.py:128``, ``fed_scr.py:126``) and on the
server's downstream (``fl_model.py:558-563``); sparse uploads ("both") need
an aggregator that takes them, ``SparsePlainAggregator``.  ``fed_scr`` (structure-wise pruning of
the upload, ``fed_scr.py:42-139``; the server passes it through,
``compress.py:56-57``) is the reference's other compression strategy and
shares ``fed_stc``'s worker flow; its kernels are ``sa_scr``'s.

``fed_smp`` is the reference's strategy that combines sparsification with
client-level DP, the scheme whose output feeds the secure aggregator: the
server draws a random mask each round, a worker masks and rescales its
update, clips and noises it with ``dp_strategy.model_gdp``, masks it again
and uploads ``old + that`` (``FedSMP_torch.py:46-141``; the server's side,
``FedSMP_server_agg_method.aggregate`` at ``:149-203``, is ``FLModel``'s
here, with any aggregator).  The mask is keyed: the server sends ``(params,
SMPMask(key, p))``, 16 bytes of mask instead of an int64 array of the
model's shape, and the worker's step is ``sfl_amd.security.privacy.smp``'s
(two streaming ``sa_smp`` passes per layer on a GPU model).
"""

from __future__ import annotations

import copy
import math
import time
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

from .. import hostpipe as H
from ..device import PYU, PYUObject, reveal
from ..security.privacy.smp import SMPMask, mask_key, smp_step
from ..utils.compressor import scr_step, stc_step
from ..utils.sparse import SparseCOO, payload_nbytes, sparse_decode, sparse_encode


def _host_array(v: torch.Tensor) -> np.ndarray:
    """A fresh host copy of a model tensor (``.cpu().numpy().copy()``): a GPU
    tensor's through pinned memory, never a pageable DMA (``hostpipe.d2h``:
    the aggregator in the same process keeps registered host buffers)."""
    v = v.detach()
    return v.numpy().copy() if v.device.type == "cpu" else H.d2h(v, pooled=False)


def _host_tensor(v: torch.Tensor) -> torch.Tensor:
    """``v.cpu()`` the same way (element types numpy lacks keep ``.cpu()``)."""
    if v.device.type == "cpu" or H.host_dtype(v) is None:
        return v.cpu()
    return torch.from_numpy(H.d2h(v, pooled=False))


def optim_wrapper(func, *args, **kwargs):
    """``optim_wrapper(optim.Adam, lr=1e-2)(params)`` (reference utils.py:23)."""

    def make(params):
        return func(params, *args, **kwargs)

    return make


class TorchModel:
    """Model builder record (reference module.py:247): extra keyword
    arguments go to ``model_fn`` (e.g. MOON's ``cosine_similarity_fn``,
    tests/ml/nn/fl/strategy/test_moon_torch.py:76-91)."""

    def __init__(self, model_fn: Callable[..., torch.nn.Module] = None, loss_fn: Callable = None,
                 optim_fn: Callable = None, metrics: Optional[list] = None, **kwargs):
        self.model_fn = model_fn
        self.loss_fn = loss_fn
        self.optim_fn = optim_fn
        self.metrics = list(metrics or [])
        self.kwargs = kwargs


class FedAvgW:
    """One party's worker for the ``fed_avg_w`` strategy."""

    def __init__(self, builder: TorchModel, device: PYU, random_seed: Optional[int] = None,
                 train_device: Optional[torch.device] = None, **kwargs):
        if random_seed is not None:
            torch.manual_seed(random_seed)
        self.device = device
        self.exe_device = torch.device(train_device) if train_device is not None else device.torch_device
        self.model = builder.model_fn(**builder.kwargs).to(self.exe_device)
        self.optimizer = builder.optim_fn(self.model.parameters())
        self.loss_fn = builder.loss_fn()
        self._x = self._y = None
        self._batch = 32
        self._pos = 0

    # ----------------------------------------------------------- data
    def set_data(self, x: np.ndarray, y: np.ndarray, batch_size: int):
        self._x = torch.as_tensor(np.asarray(x, dtype=np.float32))
        self._y = torch.as_tensor(np.asarray(y))
        self._batch = int(batch_size)
        self._pos = 0

    def steps_per_epoch(self) -> int:
        return math.ceil(len(self._x) / self._batch)

    def _reset_data_iter(self):
        self._pos = 0

    def next_batch(self):
        if self._pos >= len(self._x):
            self._pos = 0
        lo, hi = self._pos, min(len(self._x), self._pos + self._batch)
        self._pos = hi
        return self._x[lo:hi].to(self.exe_device), self._y[lo:hi].to(self.exe_device)

    # -------------------------------------------------------- weights
    def get_weights(self, return_numpy: bool = True):
        if not return_numpy:
            return {k: _host_tensor(v) for k, v in self.model.state_dict().items()}
        return [_host_array(v) for v in self.model.state_dict().values()]

    def set_weights(self, weights, model: Optional[torch.nn.Module] = None):
        model = self.model if model is None else model
        sd = model.state_dict()
        new = {}
        for (k, v), w in zip(sd.items(), weights):
            if v.device.type != "cpu":
                # a GPU model: the weights reach its device by a pinned copy
                # (hostpipe.h2d, never a pageable DMA) or device to device, so
                # load_state_dict copies on the device
                t = w.detach().to(v.device) if isinstance(w, torch.Tensor) and w.device.type != "cpu" else \
                    H.h2d(w.detach() if isinstance(w, torch.Tensor) else np.asarray(w), v.device)
                new[k] = t.to(dtype=v.dtype)
                continue
            # reference: torch.Tensor(np.copy(v)) -> float32 for float params
            w = _host_array(w) if isinstance(w, torch.Tensor) else np.array(w, copy=True)
            new[k] = torch.from_numpy(w).to(dtype=v.dtype)
        model.load_state_dict(new)

    # ------------------------------------------------------- training
    # What every strategy's train_step shares; a strategy overrides the hook
    # that differs (_loss, _train_batch) and keeps its own payload around them.
    def _begin_step(self, refresh_data: bool):
        self.model.train()
        if refresh_data:
            self._reset_data_iter()

    def _loss(self, x, y):
        return self.loss_fn(self.model(x), y)

    def _train_batch(self, x, y):
        """One local step on one batch; gives its loss."""
        self.optimizer.zero_grad()
        loss = self._loss(x, y)
        loss.backward()
        self.optimizer.step()
        return loss

    def _train(self, train_steps: int) -> int:
        """``train_steps`` batches in order through ``_train_batch``; sets
        ``last_loss`` and gives the number of samples seen."""
        num_sample = 0
        loss = None
        for _ in range(train_steps):
            x, y = self.next_batch()
            num_sample += x.shape[0]
            loss = self._train_batch(x, y)
        self.last_loss = float(loss.item()) if loss is not None else float("nan")
        return num_sample

    @staticmethod
    def _model_gdp(payload, dp_strategy):
        """The payload after the strategy's model-level DP, if it has one (fed_avg_w.py:80-85)."""
        if dp_strategy is not None and dp_strategy.model_gdp is not None:
            return dp_strategy.model_gdp(payload)
        return payload

    def train_step(self, weights, cur_steps: int, train_steps: int, refresh_data: bool = False,
                   dp_strategy=None, **kwargs):
        self._begin_step(refresh_data)
        if weights is not None:
            self.set_weights(weights)
        num_sample = self._train(train_steps)
        return self._model_gdp(self.get_weights(return_numpy=True), dp_strategy), num_sample

    def apply_weights(self, weights, **kwargs):
        if weights is not None:
            self.set_weights(weights)

    @torch.no_grad()
    def evaluate(self, x, y):
        self.model.eval()
        xt = torch.as_tensor(np.asarray(x, dtype=np.float32)).to(self.exe_device)
        yt = torch.as_tensor(np.asarray(y)).to(self.exe_device)
        out = self.model(xt)
        loss = float(self.loss_fn(out, yt).item())
        acc = float((out.argmax(1) == yt).float().mean().item())
        return loss, acc

    @torch.no_grad()
    def predict(self, x, batch_size: int = 32):
        self.model.eval()
        xt = torch.as_tensor(np.asarray(x, dtype=np.float32))
        outs = [self.model(xt[i:i + batch_size].to(self.exe_device)).cpu() for i in range(0, len(xt), batch_size)]
        return torch.cat(outs).numpy() if outs else np.zeros((0,), np.float32)


class MOON(FedAvgW):
    """One party's worker for the ``moon`` strategy (model-contrastive FL,
    sfl/ml/nn/fl/backend/torch/strategy/moon.py:27-139): local loss = task
    loss + mu * CE(cos(z, z_global) / T against cos(z, z_prev) / T) with the
    model's projection ``z`` (``model(x, return_all=True)`` -> (h, z, y)),
    the aggregated global model and the last ``model_buffer_size`` local
    models.  The aggregation itself is fed_avg_w's: ``average(weights,
    weights=num_samples)`` -- the secure aggregator's caller is unchanged."""

    def __init__(self, builder: TorchModel, device: PYU, random_seed: Optional[int] = None,
                 train_device: Optional[torch.device] = None, model_buffer_size: int = 1, **kwargs):
        super().__init__(builder, device, random_seed, train_device)
        self.model_buffer_size = int(model_buffer_size)
        self.prev_model_list: List[torch.nn.Module] = []
        self.global_model = copy.deepcopy(self.model)

    def _loss(self, x, y):  # moon.py:76-97
        _, pro1, y_pred = self.model(x, return_all=True)
        loss = self.loss_fn(y_pred, y)
        _, pro2, _ = self.global_model(x, return_all=True)
        logits = self.model.cosine_similarity_fn(pro1, pro2).reshape(-1, 1)
        for pre in self.prev_model_list:
            _, pro3, _ = pre(x, return_all=True)
            nega = self.model.cosine_similarity_fn(pro1, pro3)
            logits = torch.cat((logits, nega.reshape(-1, 1)), dim=1)
        logits = logits / self.model.temperature
        labels = torch.zeros(x.size(0), dtype=torch.long, device=x.device)
        return loss + self.model.mu * self.loss_fn(logits, labels)

    def train_step(self, weights, cur_steps: int, train_steps: int, refresh_data: bool = False,
                   dp_strategy=None, **kwargs):
        self._begin_step(refresh_data)
        if weights is not None:  # moon.py:64-72: global model <- aggregated weights, frozen
            self.set_weights(weights, model=self.global_model)
            self.global_model.eval()
            for prm in self.global_model.parameters():
                prm.requires_grad = False
            self.set_weights(weights)
        num_sample = self._train(train_steps)
        model_weights = self._model_gdp(self.get_weights(return_numpy=True), dp_strategy)
        # moon.py:115-130: keep the last model_buffer_size local models, frozen
        if len(self.prev_model_list) >= self.model_buffer_size:
            self.prev_model_list.pop(0)
        hist = copy.deepcopy(self.model)
        hist.eval()
        for prm in hist.parameters():
            prm.requires_grad = False
        self.prev_model_list.append(hist)
        return model_weights, num_sample


class FedAvgU(FedAvgW):
    """``fed_avg_u`` worker (sfl/ml/nn/fl/backend/torch/strategy/fed_avg_u.py:
    30-96): clients upload their model UPDATES (new - old weights) and apply
    the aggregated update.  The aggregator sees small signed deltas."""

    def train_step(self, updates, cur_steps: int, train_steps: int, refresh_data: bool = False,
                   dp_strategy=None, **kwargs):
        self._begin_step(refresh_data)
        if updates is not None:  # fed_avg_u.py:55-57
            self.set_weights([np.add(w, u) for w, u in zip(self.get_weights(), updates)])
        old = self.get_weights()
        num_sample = self._train(train_steps)
        client_updates = [np.subtract(n, o) for n, o in zip(self.get_weights(), old)]  # :77-80
        return self._model_gdp(client_updates, dp_strategy), num_sample

    def apply_weights(self, updates, **kwargs):
        if updates is not None:
            self.set_weights([np.add(w, u) for w, u in zip(self.get_weights(), updates)])


class FedAvgG(FedAvgW):
    """``fed_avg_g`` worker (sfl/ml/nn/fl/backend/torch/strategy/fed_avg_g.py:
    28-112): clients upload the gradients of the round and step their
    optimizer with the aggregated gradients.  As in the reference,
    ``local_gradients_sum += local_gradients`` (:91) CONCATENATES the
    per-step gradient lists, so with ``aggregate_freq = k`` the payload the
    aggregator sees is k x the parameter list (k x the mask-stream draws per
    round), and ``set_gradients`` zips it with the parameters
    (mixins.py:99-111), i.e. steps with the first local step's aggregated
    gradients.  One deviation, about the reference's plumbing rather than
    the aggregation: the aggregate (float64 out of the secure decode) is cast
    to each parameter's dtype before it becomes ``p.grad`` (the reference
    assigns it as is, which torch rejects for float32 parameters)."""

    def _set_gradients(self, gradients):
        for g, prm in zip(gradients, self.model.parameters()):
            if g is not None:
                prm.grad = torch.from_numpy(np.array(g, copy=True)).to(device=prm.device, dtype=prm.dtype)

    def _train_batch(self, x, y):
        """No optimizer step: the batch's gradients join the round's payload."""
        self.optimizer.zero_grad()
        loss = self._loss(x, y)
        loss.backward()
        grads = [None if prm.grad is None else _host_array(prm.grad)
                 for prm in self.model.parameters()]  # mixins.py:91-97
        # list += list: concatenation (:91)
        self._grad_sum = grads if self._grad_sum is None else self._grad_sum + grads
        return loss

    def train_step(self, gradients, cur_steps: int, train_steps: int, refresh_data: bool = False,
                   dp_strategy=None, **kwargs):
        self._begin_step(refresh_data)
        if gradients is not None:  # fed_avg_g.py:67-71
            self._set_gradients(gradients)
            self.optimizer.step()
        self._grad_sum = None
        num_sample = self._train(train_steps)
        return self._model_gdp(self._grad_sum, dp_strategy), num_sample

    def apply_weights(self, gradients, **kwargs):
        if gradients is not None:  # fed_avg_g.py:103-112
            self._set_gradients(gradients)
            self.optimizer.step()


class FedSTC(FedAvgW):
    """``fed_stc`` worker (sfl/ml/nn/fl/backend/torch/strategy/fed_stc.py:
    42-143): add the downstream update to the kept weights, snapshot, train,
    upload STC(new - old + residual), keep the new residual, and go back to
    the snapshot (the local step itself is discarded, as in the reference).

    ``sparsity`` is the masked fraction; ``compress_device`` says where STC
    runs (default: the training device).  With a GPU model the weights, the
    snapshot, the residual and the payload stay on the device; with a host
    model and a GPU ``compress_device`` the arrays cross through pinned
    memory (``hostpipe.h2d`` / ``d2h``) and the residual stays on the GPU."""

    def __init__(self, builder: TorchModel, device: PYU, random_seed: Optional[int] = None,
                 train_device: Optional[torch.device] = None, sparsity: float = 0.0, compress_device=None,
                 sparse_transport: Optional[str] = None, **kwargs):
        super().__init__(builder, device, random_seed, train_device)
        assert 0 <= sparsity <= 1, f"sparse rate should between 0 and 1, but get {sparsity}"
        self.sparsity = float(sparsity)
        self.sparse_transport = sparse_transport  # None / "down" / "both" (FLModel checks the value)
        self.compress_device = torch.device(compress_device) if compress_device is not None else self.exe_device
        # device-resident: a GPU model compressed on its own GPU
        self._resident = self.exe_device.type != "cpu" and self.compress_device == self.exe_device
        self._res: list = []
        self.model_weights = None

    def _state(self) -> list:
        if self._resident:
            return [v.detach().clone() for v in self.model.state_dict().values()]
        return self.get_weights()

    def _plus(self, weights, updates) -> list:
        """``np.add(w, u)`` layer by layer (fed_stc.py:72), where each lives."""
        out = []
        for w, u in zip(weights, updates):
            if self._resident:
                out.append(torch.add(w, H.h2d(u, w.device)))
            else:
                out.append(np.add(w, H.d2h(u, pooled=False) if isinstance(u, torch.Tensor) and u.is_cuda
                                  else np.asarray(u)))
        return out

    def _upload(self, payload: list) -> list:
        """What leaves the worker: with ``sparse_transport="both"`` the COO
        form of the payload (fed_stc.py:128)."""
        return sparse_encode(payload) if self.sparse_transport == "both" else payload

    @staticmethod
    def _dense(updates):
        """The downstream update, decoded if it came in COO form (fed_stc.py:71, :141)."""
        if updates is not None and any(isinstance(u, SparseCOO) for u in updates):
            return sparse_decode(updates)
        return updates

    def _step(self, a, b, r):
        """The strategy's compression of ``(a - b) + r`` where the operands live: (payload, residual)."""
        return stc_step(a, b, r, self.sparsity)[:2]

    def _compress(self, a, b, r):
        """One layer's (payload, residual).  Float layers run on
        ``compress_device``; integer entries take the numpy path."""
        if self._resident or self.compress_device.type == "cpu" or a.dtype not in (np.float32, np.float64):
            return self._step(a, b, r)
        dev = self.compress_device
        sparse, res = self._step(H.h2d(a, dev), None if b is None else H.h2d(b, dev), r)
        return H.d2h(sparse, pooled=False), res

    def train_step(self, updates, cur_steps: int, train_steps: int, refresh_data: bool = False,
                   dp_strategy=None, **kwargs):
        self._begin_step(refresh_data)
        updates = self._dense(updates)
        if updates is not None:  # fed_stc.py:69-73
            self.set_weights(self._plus(self.model_weights, updates))
        self.model_weights = self._state()  # :78
        num_sample = self._train(train_steps)
        new = self._state()
        res = self._res or [None] * len(new)
        if dp_strategy is not None and dp_strategy.model_gdp is not None:  # :113-118: DP on the dense update
            host = [_host_array(t) if isinstance(t, torch.Tensor) else t for t in (*new, *self.model_weights)]
            dense = [np.subtract(n, o) for n, o in zip(host[:len(new)], host[len(new):])]
            dense = [u if r is None else np.add(u, _host_array(r) if isinstance(r, torch.Tensor) else r)
                     for u, r in zip(dense, res)]
            dense = dp_strategy.model_gdp(dense)
            if self._resident:
                dense = [H.h2d(u, self.exe_device) for u in dense]
            pairs = [self._compress(u, None, None) for u in dense]
        else:  # :97-111, :120-125 in one step per layer
            pairs = [self._compress(n, o, r) for n, o, r in zip(new, self.model_weights, res)]
        self._res = [p[1] for p in pairs]
        self.set_weights(self.model_weights)  # :126
        return self._upload([p[0] for p in pairs]), num_sample

    def apply_weights(self, updates, **kwargs):
        updates = self._dense(updates)
        if updates is not None:  # fed_stc.py:139-143
            self.set_weights(self._plus(self.model_weights, updates))


class FedSCR(FedSTC):
    """``fed_scr`` worker (sfl/ml/nn/fl/backend/torch/strategy/fed_scr.py:
    42-139): ``FedSTC``'s flow with structure-wise pruning in place of the
    ternary compression: rows and columns of a dense layer's update, filters
    and channels of a conv layer's, whose sum of magnitudes relative to the
    largest is at most ``threshold`` are dropped
    (``sfl_amd.utils.compressor.scr_step``); other entries travel as they are.

    ``keep_residual=False`` is what the reference does: its ``SCRSparse``
    prunes the dense update in place, so the residual it forms from the two
    (fed_scr.py:120-123) is identically zero and what a worker drops is lost.
    The residual stays empty and no residual is computed.
    ``keep_residual=True`` keeps ``update - payload`` and adds it to the next
    round's update, the error feedback of the FedSCR paper."""

    def __init__(self, builder: TorchModel, device: PYU, random_seed: Optional[int] = None,
                 train_device: Optional[torch.device] = None, threshold: float = 0.0, compress_device=None,
                 keep_residual: bool = False, sparse_transport: Optional[str] = None, **kwargs):
        super().__init__(builder, device, random_seed, train_device, sparsity=0.0, compress_device=compress_device,
                         sparse_transport=sparse_transport)
        self.threshold = float(threshold)
        self.keep_residual = bool(keep_residual)

    def _step(self, a, b, r):
        return scr_step(a, b, r, self.threshold, want_res=self.keep_residual)

    def train_step(self, updates, cur_steps: int, train_steps: int, refresh_data: bool = False,
                   dp_strategy=None, **kwargs):
        out = super().train_step(updates, cur_steps, train_steps, refresh_data, dp_strategy, **kwargs)
        if not self.keep_residual:
            self._res = []
        return out


class FedSMP(FedAvgW):
    """``fed_smp`` worker (examples/security/h_gia/FedSMP_defense/
    FedSMP_torch.py:46-141): take the server's weights and mask, snapshot,
    train, and upload ``old + mask * model_gdp(mask * (new - old) /
    (compression_ratio + 1e-6))`` (``smp_step``; its docstring has the
    definition and where it departs from the reference).

    The server's message is ``(weights, SMPMask)``; ``compression_ratio`` is
    the keep probability the server draws its masks with (the divisor comes
    from the mask received, which carries the same ratio).  ``smp_device``
    says where the step runs (default: the training device).  With a GPU
    model the weights, the snapshot and the upload stay on the device; with
    a host model and a GPU ``smp_device`` the float32 layers cross through
    pinned memory (``hostpipe.h2d`` / ``d2h``)."""

    def __init__(self, builder: TorchModel, device: PYU, random_seed: Optional[int] = None,
                 train_device: Optional[torch.device] = None, compression_ratio: float = 1.0, smp_device=None,
                 **kwargs):
        super().__init__(builder, device, random_seed, train_device)
        assert 0 <= compression_ratio <= 1, f"compression ratio should between 0 and 1, but get {compression_ratio}"
        self.compression_ratio = float(compression_ratio)
        self.smp_device = torch.device(smp_device) if smp_device is not None else self.exe_device
        self._resident = self.exe_device.type != "cpu" and self.smp_device == self.exe_device
        self.grad_mask: Optional[SMPMask] = None

    def _state(self) -> list:
        if self._resident:
            return [v.detach().clone() for v in self.model.state_dict().values()]
        return self.get_weights()

    def set_weights(self, weights, model: Optional[torch.nn.Module] = None):
        if isinstance(weights, tuple) and len(weights) == 2 and isinstance(weights[1], SMPMask):  # :125-127
            weights, self.grad_mask = weights
        super().set_weights(weights, model)

    def _smp(self, old: list, new: list, model_gdp) -> list:
        if self._resident or self.smp_device.type == "cpu":
            return smp_step(old, new, self.grad_mask, model_gdp)
        dev, f32 = self.smp_device, [a.dtype == np.float32 for a in old]
        up = smp_step([H.h2d(a, dev) if f else a for a, f in zip(old, f32)],
                      [H.h2d(a, dev) if f else a for a, f in zip(new, f32)], self.grad_mask, model_gdp)
        return [H.d2h(a, pooled=False) if f else a for a, f in zip(up, f32)]

    def train_step(self, weights, cur_steps: int, train_steps: int, refresh_data: bool = False,
                   dp_strategy=None, **kwargs):
        self._begin_step(refresh_data)
        if weights is not None:  # :68-75
            self.set_weights(weights)
        if self.grad_mask is None:
            raise ValueError("fed_smp: no mask received yet; the server sends (weights, SMPMask)")
        old = self._state()  # :78
        num_sample = self._train(train_steps)
        model_gdp = dp_strategy.model_gdp if dp_strategy is not None else None
        return self._smp(old, self._state(), model_gdp), num_sample  # :105-119


_STRATEGIES = {("fed_smp", "torch"): FedSMP, ("fed_stc", "torch"): FedSTC, ("fed_scr", "torch"): FedSCR, ("fed_avg_w", "torch"): FedAvgW, ("fed_avg_u", "torch"): FedAvgU, ("fed_avg_g", "torch"): FedAvgG,
               ("moon", "torch"): MOON}


class FLModel:
    """Horizontal FL over ``device_list`` with ``aggregator`` (any object with
    the ``Aggregator`` surface: ``average(data, axis, weights)``).

    ``sparse_transport`` (``fed_stc`` / ``fed_scr`` only; default None: dense,
    as before): ``"down"`` sends the server's compressed update to the
    parties in COO form (``fed_stc``; ``fed_scr``'s downstream is not
    compressed and stays dense) and works with any aggregator; ``"both"``
    also uploads in COO form and needs an aggregator that declares
    ``accepts_sparse`` (``SparsePlainAggregator``).  When it is set,
    ``history`` has ``upload_bytes`` and ``download_bytes``, one entry per
    round: the bytes of all parties' uploads and of all parties' copies of
    the downstream payload.

    ``strategy="fed_smp"`` (``compression_ratio``, ``smp_device``): after the
    initial average and after every aggregation the server draws a fresh mask
    key and sends ``(params, SMPMask(key, compression_ratio))`` to every
    party.  Without a ``random_seed`` the key is ``secrets.randbits(64)``;
    with one, draw ``k`` (0 with the initial average) has the key
    ``sfl_amd.security.privacy.smp.mask_key(random_seed, k)``.  ``masks``
    keeps the masks drawn so far and ``history["mask_bytes"]`` the bytes of
    mask sent per round, 16 per party."""

    def __init__(self, server: Optional[PYU] = None, device_list: List[PYU] = (), model: TorchModel = None,
                 aggregator=None, strategy: str = "fed_avg_w", backend: str = "torch",
                 random_seed: Optional[int] = None, train_device=None, dp_strategy=None,
                 sparse_transport: Optional[str] = None, **kwargs):
        if (strategy, backend) not in _STRATEGIES:
            raise NotImplementedError(f"strategy {strategy!r} / backend {backend!r}")
        if aggregator is None:
            raise ValueError("this build aggregates through an Aggregator (server_agg_method is out of scope)")
        if sparse_transport is not None:
            if sparse_transport not in ("down", "both"):
                raise ValueError(f"sparse_transport is None, 'down' or 'both', not {sparse_transport!r}")
            if strategy not in ("fed_stc", "fed_scr"):
                raise ValueError(f"sparse_transport needs a compressing strategy (fed_stc, fed_scr), not {strategy!r}")
            if sparse_transport == "both" and not getattr(aggregator, "accepts_sparse", False):
                raise ValueError(
                    f"sparse_transport='both' needs an aggregator that takes sparse uploads (accepts_sparse, "
                    f"SparsePlainAggregator); {type(aggregator).__name__} does not: a secure aggregator masks "
                    f"every element, so its uploads stay dense.  sparse_transport='down' is what it can use")
            kwargs["sparse_transport"] = sparse_transport
        self.sparse_transport = sparse_transport
        self.server = server
        self.device_list = list(device_list)
        self._aggregator = aggregator
        self.strategy = strategy
        self.dp_strategy = dp_strategy
        self._random_seed = random_seed
        self._smp_ratio = float(kwargs.get("compression_ratio", 1.0))  # fed_smp: the masks' keep probability
        self.masks: List[SMPMask] = []  # fed_smp: every mask drawn, in order
        self._sparsity = float(kwargs.get("sparsity", 0.0))  # fed_stc: the server compresses at the same rate
        self._res: list = []  # fed_stc: the server's residual (fl_model.py:544-556)
        self._workers: Dict[PYU, FedAvgW] = {
            d: _STRATEGIES[(strategy, backend)](model, d, random_seed, train_device, **kwargs)
            for d in self.device_list}

    def initialize_weights(self):
        """Average the clients' initial weights through the aggregator and
        install the result on every worker (reference fl_model.py:126-138):
        one secure aggregation before the first round, which also advances
        every pair's mask streams by the model's parameter count."""
        ws = [PYUObject(d, w.get_weights()) for d, w in self._workers.items()]
        init = self._aggregator.average(ws, axis=0)
        down = self._with_mask(init)
        for d, w in self._workers.items():
            w.set_weights(reveal(down.to(d)))
        return init

    def _with_mask(self, model_params: PYUObject) -> PYUObject:
        """What the server sends down: for ``fed_smp`` the aggregate with a
        freshly drawn mask (FedSMP_torch.py:201-203, the mask as its key and
        ratio), for every other strategy the aggregate itself."""
        if self.strategy != "fed_smp":
            return model_params
        self.masks.append(SMPMask(mask_key(self._random_seed, len(self.masks)), self._smp_ratio))
        return PYUObject(model_params.device, (model_params.data, self.masks[-1]))

    def _server_stc(self, agg_data: list):
        """The ``fed_stc`` server step (fl_model.py:542-556, compress.py:28-42):
        the server adds its residual to the aggregated update, compresses it,
        keeps the new residual and adds the result to ``server_weight``, its
        own copy of the model.  Gives (the sparse update, what goes back to
        the parties: the same, or its COO form with ``sparse_transport``,
        fl_model.py:558-563)."""
        # device payloads: the server's copy follows the aggregate onto its device, layer by
        # layer (a sparse aggregator's device sums stay there, its numpy fall-backs are arrays)
        self.server_weight = [H.h2d(w, a.device) if isinstance(a, torch.Tensor) and a.is_cuda
                              and not isinstance(w, torch.Tensor) else w
                              for w, a in zip(self.server_weight, agg_data)]
        # a plain aggregator's unweighted initial average keeps the model's float32 while
        # its weighted averages are float64 (numpy's promotion): the server's copy follows
        # the aggregate's type too (a no-op with an aggregator whose results are all float64)
        self.server_weight = [w if w.dtype == a.dtype else
                              (w.to(a.dtype) if isinstance(w, torch.Tensor) else w.astype(a.dtype))
                              for w, a in zip(self.server_weight, agg_data)]
        res = self._res or [None] * len(agg_data)
        steps_out = [stc_step(a, None, r, self._sparsity, acc=w)
                     for a, r, w in zip(agg_data, res, self.server_weight)]
        self._res = [s[1] for s in steps_out]
        sparse = [s[0] for s in steps_out]
        return sparse, (sparse_encode(sparse) if self.sparse_transport is not None else sparse)

    def fit(self, x: Dict[PYU, np.ndarray], y: Dict[PYU, np.ndarray], batch_size: int = 32, epochs: int = 1,
            aggregate_freq: int = 1, validation_data=None, round_hook: Callable | None = None) -> dict:
        """``round_hook(round_index, aggregated_params)`` is called after every
        aggregation, with index -1 for the initial-weights average (the test
        oracle checks rounds with it)."""
        for d, w in self._workers.items():
            w.set_data(x[d], y[d], batch_size)
        steps = max(w.steps_per_epoch() for w in self._workers.values())
        history = {"train_loss": [], "val_loss": [], "val_accuracy": [], "aggregation_s": [], "round_s": [],
                   "init_s": 0.0, "eval_s": 0.0}
        if self.sparse_transport is not None:
            history["upload_bytes"], history["download_bytes"] = [], []
        if self.strategy == "fed_smp":
            history["mask_bytes"] = []
        # reference fit (fl_model.py:473): the initial weights are averaged
        # through the aggregator before the first epoch
        t_init = time.perf_counter()
        init = self.initialize_weights()
        history["init_s"] = time.perf_counter() - t_init
        if round_hook is not None:
            round_hook(-1, reveal(init))
        if self.strategy == "fed_stc":  # fl_model.py:475-477: the server's copy of the model
            self.server_weight = [w.detach().clone() if isinstance(w, torch.Tensor) else np.array(w, copy=True)
                                  for w in reveal(init)]
        rnd = 0
        for epoch in range(epochs):
            model_params_list = None
            for step in range(0, steps, aggregate_freq):
                t_round = time.perf_counter()
                params, nums = [], []
                for idx, (d, w) in enumerate(self._workers.items()):
                    cp = reveal(model_params_list[idx]) if model_params_list is not None else None
                    n_steps = aggregate_freq if step + aggregate_freq < steps else steps - step
                    p, n = w.train_step(cp, epoch * steps + step, n_steps, refresh_data=(step == 0),
                                        dp_strategy=self.dp_strategy)
                    params.append(PYUObject(d, p))
                    nums.append(n)
                if self.sparse_transport is not None:
                    history["upload_bytes"].append(sum(payload_nbytes(p.data) for p in params))
                t_agg = time.perf_counter()
                model_params = self._aggregator.average(params, axis=0, weights=nums)
                agg_data = reveal(model_params)
                if isinstance(agg_data, list) and any(isinstance(a, torch.Tensor) and a.is_cuda for a in agg_data):
                    torch.cuda.synchronize()
                history["aggregation_s"].append(time.perf_counter() - t_agg)
                if self.strategy == "fed_stc":
                    agg_data, down = self._server_stc(agg_data)
                    model_params = PYUObject(model_params.device, down)
                if self.sparse_transport is not None:
                    history["download_bytes"].append(len(self.device_list) * payload_nbytes(reveal(model_params)))
                model_params = self._with_mask(model_params)
                if self.strategy == "fed_smp":
                    history["mask_bytes"].append(len(self.device_list) * SMPMask.nbytes)
                model_params_list = [model_params.to(d) for d in self.device_list]
                history["round_s"].append(time.perf_counter() - t_round)
                if round_hook is not None:
                    round_hook(rnd, agg_data)
                rnd += 1
            for idx, (d, w) in enumerate(self._workers.items()):
                w.apply_weights(reveal(model_params_list[idx]))
            history["train_loss"].append(float(np.mean([w.last_loss for w in self._workers.values()])))
            if validation_data is not None:
                t_eval = time.perf_counter()
                vl, va = self.evaluate(*validation_data)
                history["eval_s"] += time.perf_counter() - t_eval
                history["val_loss"].append(vl)
                history["val_accuracy"].append(va)
        return history

    def evaluate(self, x, y):
        """Global model metrics: after ``fit`` every party holds the same
        aggregated weights, so the first worker evaluates."""
        w = next(iter(self._workers.values()))
        return w.evaluate(x, y)

    def predict(self, x: Dict[PYU, np.ndarray], batch_size: int = 32) -> Dict[PYU, PYUObject]:
        """Every party's predictions on its own data (reference fl_model.py
        ``predict``: a dict device -> PYUObject)."""
        return {d: PYUObject(d, self._workers[d].predict(x[d], batch_size)) for d in self.device_list}

    def get_weights(self, device: Optional[PYU] = None):
        d = device or self.device_list[0]
        return self._workers[d].get_weights()
