"""Filters along the time axis of a pose track: what stands between the four makers of a track (``run_interpolation``, ``retarget``,
``fit_pose`` / ``fit_bones`` over a clip, ``fit_keypoints`` over a video) and ``deform_sequence`` / ``render_sequence``.

  * ``smooth_track``     a confidence-weighted Gaussian window on SO(3): per frame and joint the chordal L2 mean of the window's
                         rotations (Markley, Cheng, Crassidis & Oshman 2007), which fills gaps and is blind to each sample's sign
  * ``one_euro_track``   the one-euro filter (Casiez, Roussel & Vogel 2012) on unit quaternions and the root translation: causal,
    ``OneEuroTrack``     for live input; ``OneEuroTrack`` holds the state and filters one frame per launch

A track is what ``playback._track`` accepts as a dict: ``'local_rotation'`` (or ``'local_rotation2'``) (T, J, 4) with
``'global_trans'`` (T, 3), (T, 1, 3) or one (1, 3) for the whole track, which passes through untouched; a leading batch axis
(B, T, J, 4) / (B, T, 3) is accepted, and the result dicts of the fit functions go in as they are (their B is the T here).
Pose quaternions are not unit in this project (FK divides by |q|^2): both filters normalise what they read and return unit
quaternions.  The result has ``local_rotation``, ``local_rotation2`` (one tensor), ``global_trans`` and ``num`` as
``run_interpolation`` returns them, plus the filter's own key, and no other key of the input: a ``d_nodes`` handed on would be stale.

One launch per call (csrc/track.hip; include/riggs_hip.h states both methods step by step, tests/track_ref.py restates them in
NumPy).  No float atomics, no read-back, no synchronisation: both can be captured next to ``fit_rays`` / ``deform_by_pose``.
Inference only.
"""
from __future__ import annotations

import math

import torch

from . import _lib as L

__all__ = ["smooth_track", "one_euro_track", "OneEuroTrack", "gaussian_taps", "MAX_RADIUS", "MAX_JOINTS"]

MAX_RADIUS = L.CONSTANTS["RIGGS_TRACK_MAX_RADIUS"]
MAX_JOINTS = L.CONSTANTS["RIGGS_TRACK_MAX_JOINTS"]
STATE_KEYS = ("rotation", "omega", "gap", "trans", "velocity", "trans_gap")


def gaussian_taps(sigma, radius=None):
    """(R, [g[0] .. g[R]]): ``g[d] = exp(-d^2 / (2 sigma^2))`` in float64; ``R = ceil(3 sigma)`` by default, 0 <= R <= MAX_RADIUS."""
    sigma = float(sigma)
    if not (sigma > 0.0 and math.isfinite(sigma)) and not (sigma == 0.0 and radius in (None, 0)):
        raise ValueError("smooth_track: sigma must be positive and finite, got %r" % (sigma,))
    R = int(math.ceil(3.0 * sigma)) if radius is None else int(radius)
    if not 0 <= R <= MAX_RADIUS:
        raise ValueError("smooth_track: radius %d is outside [0, %d]" % (R, MAX_RADIUS))
    return R, [1.0] + [math.exp(-(d * d) / (2.0 * sigma * sigma)) for d in range(1, R + 1)]


_TAPS = {}  # (device, taps) -> (the float32 taps on the device, their pinned source)


def _taps_on(taps, device):
    """The float64 taps rounded to float32, as a device tensor.  Uploaded once per device and set of taps from pinned memory,
    without blocking, and kept: a later call — one under stream capture included — issues no copy at all."""
    key = (str(device), tuple(taps))
    if key not in _TAPS:
        if len(_TAPS) >= 64:
            _TAPS.clear()
        host = torch.tensor(taps, dtype=torch.float64).to(torch.float32)
        if device.type == "cuda":
            host = host.pin_memory()
        _TAPS[key] = (host.to(device, non_blocking=True), host)
    return _TAPS[key][0]


def _aligned(t):
    t = t if t.is_contiguous() else t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _confidences(name, w, shape):
    if tuple(w.shape) != shape:
        raise L.RiggsHipError("%s has shape %s, expected %s" % (name, tuple(w.shape), shape))
    return L.require_cuda_f32(name, w.detach())


def _read(track, weights, trans_weights, what):
    """-> (rot (B,T,J,4), trans (B,T,3) or None, the translation as given where it is one for the whole track, weights (B,T,J) or
    None, trans_weights (B,T) or None, batched)."""
    if not isinstance(track, dict):
        raise TypeError("%s: a track is a dict with 'local_rotation' and 'global_trans'" % what)
    lr = track["local_rotation"] if "local_rotation" in track else track["local_rotation2"]
    lr = L.require_cuda_f32("local_rotation", lr.detach())
    if lr.dim() not in (3, 4) or lr.shape[-1] != 4:
        raise L.RiggsHipError("local_rotation has shape %s, expected (T, J, 4) or (B, T, J, 4)" % (tuple(lr.shape),))
    batched = lr.dim() == 4
    lr = _aligned(lr if batched else lr[None])
    B, T, J = (int(s) for s in lr.shape[:3])
    if not 1 <= J <= MAX_JOINTS:
        raise L.RiggsHipError("%s: %d joints, 1 to %d are supported" % (what, J, MAX_JOINTS))
    gt = L.require_cuda_f32("global_trans", track["global_trans"].detach())
    constant = None
    if gt.numel() == 3 * B * T:
        gt = gt.reshape(B, T, 3)
    elif gt.numel() in (3, 3 * B):  # one translation for the track: not filtered
        gt, constant = None, track["global_trans"]
    else:
        raise L.RiggsHipError("global_trans has shape %s, expected %s, (T, 1, 3) or (1, 3) with T = %d"
                              % (tuple(gt.shape), "(B, T, 3)" if batched else "(T, 3)", T))
    if weights is not None:
        weights = _confidences("weights", weights, (B, T, J) if batched else (T, J)).reshape(B, T, J)
    if trans_weights is not None:
        if gt is None:
            raise L.RiggsHipError("%s: trans_weights with one translation for the whole track" % what)
        trans_weights = _confidences("trans_weights", trans_weights, (B, T) if batched else (T,)).reshape(B, T)
    return lr, gt, constant, weights, trans_weights, batched


def _result(rot, trans, constant, batched, **extra):
    rot = rot if batched else rot[0]
    trans = constant if trans is None else (trans if batched else trans[0])
    out = {"local_rotation": rot, "local_rotation2": rot, "global_trans": trans, "num": int(rot.shape[-3])}
    out.update(extra)
    return out


# --------------------------------------------------------------------------- the Gaussian window
def _smooth_launch(B, T, J, R, wrap, rot, trans, weights, trans_weights, taps, rot_out, trans_out, support):
    L.check(L.lib().riggs_track_smooth(B, T, J, R, int(wrap), rot.data_ptr(), L.ptr(trans), L.ptr(weights), L.ptr(trans_weights),
                                       taps.data_ptr(), rot_out.data_ptr(), L.ptr(trans_out), support.data_ptr(), L.stream_ptr()),
            "riggs_track_smooth")


def smooth_track(track, sigma, radius=None, weights=None, trans_weights=None, wrap=False):
    """The track with every rotation replaced by the chordal mean of its window ``t - R .. t + R`` under the weights
    ``exp(-d^2 / (2 sigma^2)) * weights[s, j]``, and every translation by the weighted mean over the same window.  ``sigma`` in
    frames; ``radius`` R defaults to ``ceil(3 sigma)``, at most ``MAX_RADIUS``.  ``weights`` (T, J) / (B, T, J) are confidences: a
    sample with weight <= 0 or NaN is a gap, and so is a zero or non-finite quaternion; ``trans_weights`` (T,) / (B, T) likewise
    for the translation.  A gap's values are never used: the window's other samples fill it.  The window is clipped at the
    track's ends, or with ``wrap=True`` (a looping clip) taken modulo T, which needs ``2 R + 1 <= T``.

    The extra key ``support`` (…, T, J) is the window's total weight: 0 where it held no valid sample.  There the rotation is the
    input normalised (the identity where that is zero or not finite) and the translation the input row.  Where sample (t, j) is
    valid, the output lies in its hemisphere (``dot >= 0``); else its first non-zero component is positive.  ``radius=0`` returns
    the normalised input."""
    R, taps = gaussian_taps(sigma, radius)
    rot, trans, constant, weights, trans_weights, batched = _read(track, weights, trans_weights, "smooth_track")
    B, T, J = (int(s) for s in rot.shape[:3])
    if wrap and T > 0 and 2 * R + 1 > T:
        raise ValueError("smooth_track: wrap=True needs 2 * radius + 1 <= T, got radius %d and T = %d" % (R, T))
    taps = _taps_on(taps, rot.device)
    rot_out, support = torch.empty_like(rot), torch.empty(B, T, J, dtype=torch.float32, device=rot.device)
    trans_out = None if trans is None else torch.empty_like(trans)
    _smooth_launch(B, T, J, R, bool(wrap), rot, trans, weights, trans_weights, taps, rot_out, trans_out, support)
    return _result(rot_out, trans_out, constant, batched, support=support if batched else support[0])


# --------------------------------------------------------------------------- the one-euro filter
def _fresh_state(B, J, device):
    f32 = dict(dtype=torch.float32, device=device)
    i32 = dict(dtype=torch.int32, device=device)
    rot = torch.zeros(B, J, 4, **f32)
    rot[..., 0] = 1.0
    return {"rotation": rot, "omega": torch.zeros(B, J, **f32), "gap": torch.full((B, J), -1, **i32),
            "trans": torch.zeros(B, 3, **f32), "velocity": torch.zeros(B, 3, **f32), "trans_gap": torch.full((B,), -1, **i32)}


def _check_state(state, B, J, device):
    shapes = {"rotation": (B, J, 4), "omega": (B, J), "gap": (B, J), "trans": (B, 3), "velocity": (B, 3), "trans_gap": (B,)}
    for k in STATE_KEYS:
        t = state[k]
        want = torch.int32 if k.endswith("gap") else torch.float32
        if not (t.device == device and t.dtype is want and t.is_contiguous() and tuple(t.shape) == shapes[k]):
            raise L.RiggsHipError("one-euro state '%s' must be a contiguous %s tensor of shape %s on %s" % (k, want, shapes[k], device))
    if state["rotation"].data_ptr() % 16:
        raise L.RiggsHipError("one-euro state 'rotation' must be 16-byte aligned")


def _params(rate, min_cutoff, beta, d_cutoff, trans_min_cutoff, trans_beta):
    p = (float(rate), float(min_cutoff), float(beta), float(d_cutoff),
         float(min_cutoff if trans_min_cutoff is None else trans_min_cutoff), float(beta if trans_beta is None else trans_beta))
    ok = all(math.isfinite(v) for v in p) and p[0] > 0 and p[1] > 0 and p[2] >= 0 and p[3] > 0 and p[4] > 0 and p[5] >= 0
    if not ok:
        raise ValueError("one-euro filter: rate, min_cutoff, d_cutoff and trans_min_cutoff must be positive, beta and trans_beta not "
                         "negative, all finite; got %r" % (p,))
    return p


def _euro_launch(B, T, J, rot, trans, weights, trans_weights, params, state, rot_out, trans_out):
    L.check(L.lib().riggs_track_one_euro(B, T, J, rot.data_ptr(), L.ptr(trans), L.ptr(weights), L.ptr(trans_weights), *params,
                                         state["rotation"].data_ptr(), state["omega"].data_ptr(), state["gap"].data_ptr(),
                                         state["trans"].data_ptr(), state["velocity"].data_ptr(), state["trans_gap"].data_ptr(),
                                         rot_out.data_ptr(), L.ptr(trans_out), L.stream_ptr()), "riggs_track_one_euro")


def _one_euro(track, params, weights, trans_weights, state, in_place):
    rot, trans, constant, weights, trans_weights, batched = _read(track, weights, trans_weights, "one_euro_track")
    B, T, J = (int(s) for s in rot.shape[:3])
    if state is None:
        state = _fresh_state(B, J, rot.device)
    else:
        _check_state(state, B, J, rot.device)
        if not in_place:
            state = {k: state[k].clone() for k in STATE_KEYS}
    rot_out = torch.empty_like(rot)
    trans_out = None if trans is None else torch.empty_like(trans)
    _euro_launch(B, T, J, rot, trans, weights, trans_weights, params, state, rot_out, trans_out)
    return _result(rot_out, trans_out, constant, batched, state=state)


def one_euro_track(track, rate, min_cutoff=1.0, beta=0.0, d_cutoff=1.0, trans_min_cutoff=None, trans_beta=None, weights=None,
                   trans_weights=None, state=None):
    """The one-euro filter along the track, one launch for all frames: a first-order low-pass whose cutoff
    ``min_cutoff + beta * speed`` rises with the filtered speed (rad/s for a joint, units/s for the translation), so a pose at
    rest is held steady and a fast move is followed without lag.  ``rate`` in frames per second; ``d_cutoff`` filters the speed.
    The translation's parameters default to the rotation's.  ``weights`` / ``trans_weights`` as in ``smooth_track``: a gap frame
    outputs the held value and lengthens the next step's ``dt``; before a joint's first sample the output is (1, 0, 0, 0) (the
    origin for the translation).

    ``state``: the ``"state"`` of an earlier call's result, to continue that track: filtering T frames in one call and in two calls
    with the state carried over runs the same code and gives the same bits.  It is a dict of device tensors that is never read
    back; the one passed in is left as it was."""
    return _one_euro(track, _params(rate, min_cutoff, beta, d_cutoff, trans_min_cutoff, trans_beta), weights, trans_weights, state, False)


class OneEuroTrack:
    """The streaming form: holds the state of one skeleton's filter (``J`` joints) on the device, ``filter(pose)`` is one launch for
    one frame.  The state tensors are updated in place, so a captured graph that contains ``filter`` replays correctly."""

    def __init__(self, J, rate, min_cutoff=1.0, beta=0.0, d_cutoff=1.0, trans_min_cutoff=None, trans_beta=None, device="cuda"):
        if not 1 <= int(J) <= MAX_JOINTS:
            raise L.RiggsHipError("OneEuroTrack: %d joints, 1 to %d are supported" % (J, MAX_JOINTS))
        self.J, self.params = int(J), _params(rate, min_cutoff, beta, d_cutoff, trans_min_cutoff, trans_beta)
        self.state = _fresh_state(1, self.J, device)

    def reset(self):
        """Forget every sample (in place)."""
        fresh = _fresh_state(1, self.J, self.state["gap"].device)
        for k in STATE_KEYS:
            self.state[k].copy_(fresh[k])

    def filter(self, pose, weights=None, trans_weight=None):
        """``pose``: ``'local_rotation'`` (J, 4) and ``'global_trans'`` (1, 3) or (3,) of one frame; ``weights`` (J,) and
        ``trans_weight`` (1,) device tensors or None.  -> the filtered pose under the same two keys, shapes (J, 4) and (1, 3)."""
        lr = pose["local_rotation"] if "local_rotation" in pose else pose["local_rotation2"]
        track = {"local_rotation": lr.reshape(1, self.J, 4), "global_trans": pose["global_trans"].reshape(1, 3)}
        out = _one_euro(track, self.params, None if weights is None else weights.reshape(1, self.J),
                        None if trans_weight is None else trans_weight.reshape(1), self.state, True)
        return {"local_rotation": out["local_rotation"][0], "global_trans": out["global_trans"]}
