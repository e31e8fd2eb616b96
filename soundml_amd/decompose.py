"""Decompose on MI355X: non-negative matrix factorisation of a magnitude spectrogram by multiplicative updates (Lee & Seung 2001;
Fevotte & Idier 2011), exported flat as ``nmf`` / ``nmf_activations`` / ``nmf_reconstruct`` / ``nmf_divergence``.  The reference has
no such module; the parameters carry scikit-learn's and librosa's names.

    V = Stft.power_spectrum(cfg, x) ** 0.5                                 # [...; F; T] >= 0, on the device
    W, H = nmf(V, 16, n_iter=100, beta="kullback-leibler")                 # [...; F; 16] templates, [...; 16; T] activations
    H = nmf_activations(V, W_dict, n_iter=50)                              # W fixed: per clip, or ONE dictionary [F; K] for the batch
    X = nmf_reconstruct(W, H, components=[0, 3])                           # [...; F; T]: the sum of the listed components
    M = Decompose.mask(W, H, [0, 3])                                       # that sum over floor(the sum of all): feeds Stft.invert
    obj = nmf_divergence(V, W, H, beta="kullback-leibler")                 # [...; 1]: the objective per clip, float64 inside

Shapes are feature-major with frames last; ``V``, ``W`` and ``H`` share the leading axes (the clips).  Results have the dtype of
``V``: float32 runs a float32 interior on the matrix cores, a host float64 array the same formulas in float64; device-resident
float64 is refused.  Every inner product is one chain of fused multiply-adds in one stated order (DESIGN.md 4.8i;
include/soundml_amd.h words the definition), so the tile kernels, the general kernels, a leading slice of a batch and a run
continued from its own factors give the same bits.  Device tensors run on the caller's stream and nothing synchronises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, lib
from ._tensor import OUT, STREAM, Batch, is_device, is_torch, out_ptr, prod, refuse_device_float64


def _caps():
    tile, most = C.c_int64(), C.c_int64()
    check(lib.smx_nmf_tile_cap(C.byref(tile), C.byref(most)))
    return int(tile.value), int(most.value)


TILE_K, MAX_K = _caps()             # the largest K of the tile kernels, and of any call
EPS = 2.0 ** -23


def _beta(name, beta):
    try:
        return _lib.BETA[beta]
    except (KeyError, TypeError):
        raise _lib.InvalidArgument("%s: unknown beta %r (one of %s)" % (name, beta, ", ".join(sorted(_lib.BETA)))) from None


def initial(lead, F: int, T: int, K: int, seed: int = 0):
    """The default initial factors ``(W0 [lead; F; K], H0 [lead; K; T])`` on the host in float64: ``1.0 - random`` of
    ``Generator(PCG64([seed, 0]))`` and of ``PCG64([seed, 1])``, values in (0, 1] (an exact zero would stay zero under the
    updates), drawn in C order: a leading slice of a batch starts from the batch's factors."""
    lead = tuple(int(n) for n in lead)
    W0 = 1.0 - np.random.Generator(np.random.PCG64([int(seed), 0])).random(lead + (int(F), int(K)))
    H0 = 1.0 - np.random.Generator(np.random.PCG64([int(seed), 1])).random(lead + (int(K), int(T)))
    return W0, H0


class _Spectrogram(Batch):
    """V [...; F; T]: a device view whose rows are a pitch apart and whose clips are one stride apart is taken as it stands
    (``S[..., :, a:b]``); anything else is made dense."""

    def __init__(self, V, name):
        if len(tuple(V.shape)) < 2:
            raise _lib.InvalidArgument("%s: V has rank %d (a spectrogram is [...; F; T]: at least 2)" % (name, len(tuple(V.shape))))
        self.view = None
        if is_device(V) and V.dtype.is_floating_point and V.dtype.itemsize == 4 and V.numel() > 0:
            shape, stride = tuple(V.shape), tuple(V.stride())
            lead = [(n, s) for n, s in zip(shape[:-2], stride[:-2]) if n != 1]
            nested = all(lead[i][1] == lead[i + 1][0] * lead[i + 1][1] for i in range(len(lead) - 1))
            clip = lead[-1][1] if lead else shape[-2] * stride[-2]
            if (shape[-1] == 1 or stride[-1] == 1) and stride[-2] >= shape[-1] and nested and clip >= (shape[-2] - 1) * stride[-2] + shape[-1]:
                self.view = (V, int(clip), int(stride[-2]))
        super().__init__(V if self.view is None else V[..., :1, :1], name)
        self.shape = tuple(V.shape)
        self.F, self.T = int(self.shape[-2]), int(self.shape[-1])
        self.lead_shape = self.shape[:-2]
        self.clips = prod(self.lead_shape)

    def placed(self):
        """(pointer, clip stride, row pitch) in elements"""
        if self.view is not None:
            V, clip, pitch = self.view
            return C.c_void_p(V.data_ptr()), clip, pitch
        return self.ptr(), self.F * self.T, self.T


def _factor(name, b, x, shape, what):
    """x on V's side in V's dtype, dense, of this shape"""
    if tuple(x.shape) != tuple(shape):
        raise _lib.InvalidArgument("%s: %s has shape %s where V, K and the leading axes ask for %s" % (name, what, list(x.shape), list(shape)))
    if b.device:
        import torch
        if not is_torch(x):
            x = torch.from_numpy(np.ascontiguousarray(x))
        return x.to(device=b.data.device, dtype=b.data.dtype).contiguous()
    a = x.detach().cpu().numpy() if is_torch(x) else np.asarray(x)
    return np.ascontiguousarray(a, dtype=b.data.dtype)


def _ptr(x):
    return out_ptr(x)


def nmf(V, n_components: int, n_iter: int = 100, beta: str = "frobenius", W0=None, H0=None, seed: int = 0):
    """``V [...; F; T] ~ W [...; F; K] H [...; K; T]`` after ``n_iter`` rounds of the multiplicative updates for the Frobenius
    or the Kullback-Leibler objective, each round the H update and then the W update.  ``None`` factors come from ``initial``,
    cast to the dtype of ``V``; ``n_iter = 0`` returns the initial factors.  A clip whose ``V`` holds a NaN comes out NaN in
    both factors from the second round on, and no other clip is touched."""
    name = "nmf"
    K, n_iter, code = int(n_components), int(n_iter), _beta(name, beta)
    if len(tuple(V.shape)) < 2:
        raise _lib.InvalidArgument("%s: V has rank %d (a spectrogram is [...; F; T]: at least 2)" % (name, len(tuple(V.shape))))
    F, T = int(V.shape[-2]), int(V.shape[-1])
    wide = str(getattr(V, "dtype", "")).endswith("float64")
    check((lib.smx_nmf_f64 if wide else lib.smx_nmf_f32)(None, None, None, 0, F, T, K, n_iter, code, None, None))
    b = _Spectrogram(V, name)
    refuse_device_float64(name, b, "spectrograms are")
    lead = b.lead_shape
    if W0 is None or H0 is None:
        w, h = initial(lead, F, T, K, seed)
        W0, H0 = (w if W0 is None else W0), (h if H0 is None else H0)
    W0, H0 = _factor(name, b, W0, lead + (F, K), "W0"), _factor(name, b, H0, lead + (K, T), "H0")
    return b.run((lib.smx_nmf_f32, lib.smx_nmf_f64), (b.ptr(), _ptr(W0), _ptr(H0), b.clips, F, T, K, n_iter, code, OUT, OUT),
                 lib.smx_nmf_vram_f32, (*b.placed(), _ptr(W0), F * K, _ptr(H0), K * T, b.clips, F, T, K, n_iter, code, OUT, F * K, OUT, K * T, STREAM),
                 [lead + (F, K), lead + (K, T)], skip=b.clips == 0)


def nmf_activations(V, W, n_iter: int = 100, beta: str = "frobenius", H0=None, seed: int = 0):
    """The activations ``H [...; K; T]`` of ``V`` against fixed templates: only the H update runs.  ``W`` is per clip
    ``[...; F; K]`` or ONE dictionary ``[F; K]`` for the whole batch (transcription against a template dictionary)."""
    name = "nmf_activations"
    n_iter, code = int(n_iter), _beta(name, beta)
    if len(tuple(V.shape)) < 2 or len(tuple(W.shape)) < 2:
        raise _lib.InvalidArgument("%s: V and W have ranks %d and %d (at least 2)" % (name, len(tuple(V.shape)), len(tuple(W.shape))))
    F, T, K = int(V.shape[-2]), int(V.shape[-1]), int(W.shape[-1])
    wide = str(getattr(V, "dtype", "")).endswith("float64")
    check((lib.smx_nmf_activations_f64 if wide else lib.smx_nmf_activations_f32)(None, None, None, 0, F, T, K, n_iter, code, None))
    b = _Spectrogram(V, name)
    refuse_device_float64(name, b, "spectrograms are")
    lead = b.lead_shape
    shared = len(lead) > 0 and tuple(W.shape) == (F, K)
    if not shared and tuple(W.shape[:-2]) != lead:
        raise _lib.InvalidArgument("%s: the leading axes of V are %s and those of W are %s (the clips must agree, or W is one [F; K])" % (
            name, list(lead), list(W.shape[:-2])))
    W = _factor(name, b, W, ((F, K) if shared else lead + (F, K)), "W")
    if H0 is None:
        H0 = initial(lead, F, T, K, seed)[1]
    H0 = _factor(name, b, H0, lead + (K, T), "H0")
    stride = 0 if shared else F * K
    if shared and not b.device and b.clips:              # the host face takes a dictionary per clip
        W = np.ascontiguousarray(np.broadcast_to(W, lead + (F, K)))
    return b.run((lib.smx_nmf_activations_f32, lib.smx_nmf_activations_f64), (b.ptr(), _ptr(W), _ptr(H0), b.clips, F, T, K, n_iter, code, OUT),
                 lib.smx_nmf_activations_vram_f32, (*b.placed(), _ptr(W), stride, _ptr(H0), K * T, b.clips, F, T, K, n_iter, code, OUT, K * T, STREAM),
                 lead + (K, T), skip=b.clips == 0)


def _factors(name, W, H):
    sw, sh = tuple(W.shape), tuple(H.shape)
    if len(sw) < 2 or len(sh) < 2:
        raise _lib.InvalidArgument("%s: W and H have ranks %d and %d (at least 2)" % (name, len(sw), len(sh)))
    if sw[-1] != sh[-2]:
        raise _lib.InvalidArgument("%s: W has %d components and H has %d" % (name, sw[-1], sh[-2]))
    if sw[:-2] != sh[:-2]:
        raise _lib.InvalidArgument("%s: the leading axes of W are %s and those of H are %s (the clips must agree)" % (
            name, list(sw[:-2]), list(sh[:-2])))
    return int(sw[-2]), int(sh[-1]), int(sw[-1])


def _reconstruct(name, W, H, components, as_mask):
    F, T, K = _factors(name, W, H)
    if components is None:
        comps, count = None, 0
    else:
        idx = [int(k) for k in components]
        comps, count = (C.c_int64 * max(1, len(idx)))(*idx), len(idx)
    wide = str(getattr(H, "dtype", "")).endswith("float64")
    check((lib.smx_nmf_reconstruct_f64 if wide else lib.smx_nmf_reconstruct_f32)(None, None, 0, F, T, K, comps, count, as_mask, None))
    b = Batch(H, name)
    refuse_device_float64(name, b, "factors are")
    lead = b.shape[:-2]
    W = _factor(name, b, W, lead + (F, K), "W")
    clips = prod(lead)
    return b.run((lib.smx_nmf_reconstruct_f32, lib.smx_nmf_reconstruct_f64), (_ptr(W), b.ptr(), clips, F, T, K, comps, count, as_mask, OUT),
                 lib.smx_nmf_reconstruct_vram_f32, (_ptr(W), F * K, b.ptr(), K * T, clips, F, T, K, comps, count, as_mask, OUT, F * T, T, STREAM),
                 lead + (F, T), skip=clips == 0, overwritten=True)


def nmf_reconstruct(W, H, components=None):
    """``W H`` [...; F; T] by the chain over the components that the updates use; with a list of component indices only those
    enter the sum (in ascending order, whatever the list's)."""
    return _reconstruct("nmf_reconstruct", W, H, components, 0)


def mask(W, H, components):
    """The soft mask of the listed components, ``reconstruct(components) / floor(reconstruct(all))`` [...; F; T]: multiplied
    into the complex spectrum it feeds ``Stft.invert`` (component-wise resynthesis)."""
    return _reconstruct("nmf_mask", W, H, components, 1)


def nmf_divergence(V, W, H, beta: str = "frobenius"):
    """The objective per clip [...; 1], float64 inside with ``X = W H`` from the stored factors: Frobenius
    ``sqrt(sum (V - X)^2 / sum V^2)``, Kullback-Leibler ``(sum_{V > 0} V log(V / X) - sum V + sum X) / sum V``."""
    name = "nmf_divergence"
    code = _beta(name, beta)
    F, T, K = _factors(name, W, H)
    if len(tuple(V.shape)) < 2 or (int(V.shape[-2]), int(V.shape[-1])) != (F, T):
        raise _lib.InvalidArgument("%s: V has shape %s where the factors give [...; %d; %d]" % (name, list(V.shape), F, T))
    if tuple(V.shape[:-2]) != tuple(H.shape[:-2]):
        raise _lib.InvalidArgument("%s: the leading axes of V are %s and those of H are %s (the clips must agree)" % (
            name, list(V.shape[:-2]), list(H.shape[:-2])))
    wide = str(getattr(V, "dtype", "")).endswith("float64")
    check((lib.smx_nmf_divergence_f64 if wide else lib.smx_nmf_divergence_f32)(None, None, None, 0, F, T, K, code, None))
    b = _Spectrogram(V, name)
    refuse_device_float64(name, b, "spectrograms are")
    lead = b.lead_shape
    W, H = _factor(name, b, W, lead + (F, K), "W"), _factor(name, b, H, lead + (K, T), "H")
    return b.run((lib.smx_nmf_divergence_f32, lib.smx_nmf_divergence_f64), (b.ptr(), _ptr(W), _ptr(H), b.clips, F, T, K, code, OUT),
                 lib.smx_nmf_divergence_vram_f32, (*b.placed(), _ptr(W), F * K, _ptr(H), K * T, b.clips, F, T, K, code, OUT, STREAM),
                 lead + (1,), skip=b.clips == 0)


reconstruct, activations, divergence = nmf_reconstruct, nmf_activations, nmf_divergence
