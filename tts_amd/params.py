"""Build nn.Module trees whose ``state_dict`` keys equal the reference checkpoint keys.

The modules only hold parameters (PyTorch is plumbing here: device memory, ``.cuda()``,
``load_state_dict``); all compute goes through ``libttship.so``.
"""

import itertools

import numpy as np
import torch
from torch import nn

from . import _lib

BUFFER_KINDS = {"bn_mean", "bn_var", "count", "buffer"}


class Container(nn.Module):
    """Plain parameter holder (one level of a dotted state_dict key)."""

    def forward(self, *args, **kwargs):  # pragma: no cover - never called
        raise RuntimeError("parameter container; use the model's inference()")


def child(root: nn.Module, path):
    m = root
    for p in path:
        if p not in m._modules:
            m.add_module(p, Container())
        m = m._modules[p]
    return m


def populate(root: nn.Module, spec, skip_prefixes=()):
    """Register every (name, shape, kind) of ``spec`` under ``root`` (zeros; loaded later)."""
    for name, shape, kind in spec:
        if any(name.startswith(p) for p in skip_prefixes):
            continue
        *path, leaf = name.split(".")
        m = child(root, path)
        if kind == "count":
            m.register_buffer(leaf, torch.zeros(shape, dtype=torch.long))
        elif kind in BUFFER_KINDS:
            m.register_buffer(leaf, torch.zeros(shape, dtype=torch.float32))
        else:
            setattr(m, leaf, nn.Parameter(torch.zeros(shape, dtype=torch.float32), requires_grad=False))
    return root


def host_tensors(module: nn.Module, skip_prefixes=(), skip_kinds=("num_batches_tracked",)):
    """state_dict as contiguous fp32 numpy arrays (what the C ABI's set_tensor takes)."""
    out = {}
    for k, v in module.state_dict().items():
        if any(k.startswith(p) for p in skip_prefixes) or k.split(".")[-1] in skip_kinds:
            continue
        out[k] = v.detach().to("cpu", torch.float32).contiguous().numpy()
    return out


def row_lengths(lengths, B, T, name):
    """Per-row lengths of a padded (B, T) batch as int64 numpy: ``lengths``, or T for every row."""
    lens = np.full(B, T, np.int64) if lengths is None else np.asarray(torch.as_tensor(lengths).cpu(), dtype=np.int64)
    if len(lens) != B or lens.min() < 1 or lens.max() > T:
        raise ValueError(f"{name} must have B entries in [1, T]")
    return lens


_TOKENS = itertools.count(1)


def new_token() -> int:
    """Process-unique model identity for the engine's weight cache (never reused, unlike id())."""
    return next(_TOKENS)


class NativeModel(nn.Module):
    """Base of every model whose weights the library packs into a device-side slot of the Engine.

    The engine remembers, per slot, the ``weight_key`` of the model it last loaded; ``_sync`` uploads
    again when that differs. Anything that changes parameters or their placement bumps the key. A
    subclass sets ``_slot`` and writes ``_load`` (its one ``eng.load_*`` call)."""

    _slot = None

    def __init__(self):
        super().__init__()
        # not named _version: nn.Module._version is the state_dict format version torch saves
        self._weights_version = 0
        self._token = new_token()
        self._device = None

    @property
    def weight_key(self):
        return self._token, self._weights_version

    @property
    def device(self):
        """All parameters move together (``_apply``), so the first one's device is the model's.
        Looked up once per weight version: every call asks, and walking the module tree is not free."""
        if self._device is None:
            self._device = next(self.parameters()).device
        return self._device

    def invalidate(self):
        """Call after editing parameters in place: the packed device copy is stale."""
        self._weights_version += 1
        self._device = None

    def _engine(self):
        return _lib.get_engine(self.device)  # looked up at call time: tests replace _lib.get_engine

    def load_state_dict(self, state_dict, strict=True, **kw):
        res = super().load_state_dict(state_dict, strict=strict, **kw)
        self.invalidate()
        return res

    def _apply(self, fn, *args, **kwargs):
        res = super()._apply(fn, *args, **kwargs)
        self.invalidate()
        return res

    def _load(self, eng):
        raise NotImplementedError

    def _sync(self, eng):
        """Upload the weights unless the engine holds them already (caller holds ``eng.lock``)."""
        if eng.weight_keys.get(self._slot) != self.weight_key:
            eng.weight_keys[self._slot] = None  # a load that fails has already dropped the old weights
            self._load(eng)
            eng.weight_keys[self._slot] = self.weight_key

    def _fold_weight_norm(self, paths):
        """Fold w = g * v / ||v|| into ``weight`` for the weight-normed module at each dotted path."""
        if not self._wn:
            return
        for path in paths:
            m = self.get_submodule(path)
            w = torch._weight_norm(m.weight_v.data, m.weight_g.data, 0)
            del m._parameters["weight_g"]
            del m._parameters["weight_v"]
            m.weight = nn.Parameter(w.contiguous(), requires_grad=False)
        self._wn = False
        self.invalidate()
