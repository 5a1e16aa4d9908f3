"""Window / rollout driver around the sampler (reference: sample_utils.py:279-375, `fill_latent` and `do_sample`).

BASELINE config 4 (long-horizon rollout): round 0 predicts a 25-frame window from the initial conditioning frame(s); every
later round re-conditions on the last three frames of the previous window (their latents are carried over as cond frames,
the decoded third-from-last frame feeds the image embedder) and contributes `num_frames - 3` new frames.

`model` is duck-typed like the reference's DiffusionEngine -- `VistaPipeline` below bundles the vista_amd pieces that way:
    model.model / model.denoiser        network wrapper and Denoiser (called as model.denoiser(model.model, x, sigma, cond, mask))
    model.decode_first_stage(z)         latents -> images            model.encode_first_stage(x)   images -> latents
    model.scale_factor                  model.conditioner.embedders  (skip_encode toggling)        model.ema_scope(...)
The conditioner (vista_amd.modules.encoders.modules.GeneralConditioner: OpenCLIP image tower, first-stage encoder, sinusoid embedders --
SURVEY.md 8f rank 2) plugs in as `VistaPipeline(conditioner=...)`: `get_condition` / `get_batch` below are the reference's
(sample_utils.py:232-276). A caller may still pass its own `get_condition` (same signature) or give the pipeline a `condition_fn`.
"""
import math
import contextlib

import torch

from .models.diffusion import decode_first_stage as _decode_first_stage
from .modules.diffusionmodules.denoiser import Denoiser
from .modules.diffusionmodules.sampling import FusedDenoiser


def fill_latent(cond, length, cond_indices, device):
    """A `length`-frame latent stack that is zero except for `cond` at `cond_indices` (sample_utils.py:279-282)."""
    latent = torch.zeros((length,) + tuple(cond.shape[1:]), device=device, dtype=cond.dtype)
    latent[cond_indices] = cond.to(device)
    return latent


class VistaPipeline:
    """The attributes of DiffusionEngine that `do_sample` touches, over vista_amd modules."""

    def __init__(self, network, denoiser, decoder=None, encode_fn=None, condition_fn=None, scale_factor=0.18215,
                 en_and_decode_n_samples_a_time=14, conditioner=None):
        self.model, self.denoiser = network, denoiser
        self.decoder, self.encode_fn, self.condition_fn = decoder, encode_fn, condition_fn
        self.scale_factor = scale_factor
        self.en_and_decode_n_samples_a_time = en_and_decode_n_samples_a_time
        self.conditioner = conditioner if conditioner is not None else _NoEmbedders()
        if conditioner is not None and condition_fn is None:
            self.condition_fn = get_condition

    def ema_scope(self, *_a, **_k):
        return contextlib.nullcontext()

    def decode_first_stage(self, z, overlap=3):
        if self.decoder is None:
            raise RuntimeError("VistaPipeline: no first-stage decoder was given")
        return _decode_first_stage(self.decoder, z, self.scale_factor, self.en_and_decode_n_samples_a_time, overlap)

    def encode_first_stage(self, x):
        if self.encode_fn is None:
            raise RuntimeError("VistaPipeline: no first-stage encoder was given (pass latents through encode_fn=lambda x: x)")
        return self.encode_fn(x)


class _NoEmbedders:
    embedders = ()


def get_batch(keys, value_dict, N, device="cuda"):
    """sample_utils.py:232-253: per-key batch tensors of the demo setups -- scalars (fps_id, motion_bucket_id, cond_aug) repeated prod(N)
    times, action vectors and conditioning frames repeated N[0] times; batch_uc is a clone."""
    batch = {}
    for key in keys:
        if key not in value_dict:
            continue
        if key in ("fps", "fps_id", "motion_bucket_id", "cond_aug"):
            batch[key] = torch.tensor([value_dict[key]]).to(device).repeat(math.prod(N))
        elif key in ("command", "trajectory", "speed", "angle", "goal"):
            v = value_dict[key][None].to(device)
            batch[key] = v.repeat(N[0], *([1] * (v.dim() - 1)))
        elif key in ("cond_frames", "cond_frames_without_noise"):
            v = value_dict[key]
            batch[key] = v.repeat(N[0], *([1] * (v.dim() - 1)))
        else:
            raise NotImplementedError(key)
    batch_uc = {k: torch.clone(v) for k, v in batch.items() if isinstance(v, torch.Tensor)}
    return batch, batch_uc


def get_condition(model, value_dict, num_samples, force_uc_zero_embeddings, device):
    """sample_utils.py:256-276 (without the load_model / unload_model host<->device shuffling: 288 GB of HBM keep the conditioner resident)."""
    keys = list({e.input_key for e in model.conditioner.embedders if getattr(e, "input_key", None) is not None})
    batch, batch_uc = get_batch(keys, value_dict, [num_samples], device)
    c, uc = model.conditioner.get_unconditional_conditioning(batch, batch_uc=batch_uc, force_uc_zero_embeddings=force_uc_zero_embeddings)
    for k in c:
        if isinstance(c[k], torch.Tensor):
            c[k], uc[k] = c[k][:num_samples].to(device), uc[k][:num_samples].to(device)
            if c[k].shape[0] < num_samples:
                c[k] = c[k][[0]]
            if uc[k].shape[0] < num_samples:
                uc[k] = uc[k][[0]]
    return c, uc


def _set_skip_encode(model, flag):
    for emb in model.conditioner.embedders:
        if hasattr(emb, "skip_encode"):
            emb.skip_encode = flag


CARRY = 3   # frames handed from one window to the next


def rollout_denoiser(model, fused=True):
    """What a sampling round hands the sampler: the reference's closure (sample_utils.py:314-315), or a FusedDenoiser over the same two objects."""
    def denoiser(x, sigma, cond, cond_mask):
        return model.denoiser(model.model, x, sigma, cond, cond_mask)
    if fused and isinstance(model.denoiser, Denoiser):
        denoiser = FusedDenoiser(model.denoiser, model.model)
    return denoiser


def rollout_masks(num_frames, initial_cond_indices, device):
    """-> (the first round's conditioning mask, every later round's: the carried frames)."""
    first_mask = torch.zeros(num_frames, device=device)
    first_mask[initial_cond_indices] = 1
    carry_mask = torch.zeros(num_frames, device=device)
    carry_mask[:CARRY] = 1
    return first_mask, carry_mask


def first_round(sampler, denoiser, c, uc, z, first_mask, noise_fn):
    """Round 0: the window grows out of the initial conditioning frame(s); the sampler rescales cond_frame itself."""
    sample = sampler(denoiser, noise_fn(z), cond=c, uc=uc, cond_frame=z, cond_mask=first_mask)
    sample[0] = z[0]
    return sample


def next_round_inputs(model, sample, num_frames, device):
    """What a later round takes from the previous window `sample`, whatever its action -> (cond_frames_without_noise: the decoded
    third-from-last frame, for the image embedder; cond_frames: its latent, for the concat conditioning (no re-encode); seeded: the last three
    latents as the conditioning frames of a zero window). One 14-frame decode."""
    tail_images = model.decode_first_stage(sample[-14:])
    seeded = fill_latent(sample[-CARRY:], num_frames, list(range(CARRY)), device)
    return tail_images[[-CARRY]], sample[[-CARRY]] / model.scale_factor, seeded


def next_round_condition(model, value_dict, num_frames, get_condition, force_uc_zero_embeddings, device):
    """(c, uc) of a later round: `value_dict` holds the round's scalars and action and next_round_inputs' two conditioning frames; the first
    stage embedder takes its frame as the latent it already is (skip_encode)."""
    _set_skip_encode(model, True)
    try:
        return get_condition(model, value_dict, num_frames, force_uc_zero_embeddings, device)
    finally:
        _set_skip_encode(model, False)


def next_round(model, sampler, denoiser, value_dict, sample, num_frames, carry_mask, get_condition, force_uc_zero_embeddings, device, noise_fn):
    """A later round from the previous window `sample`: the decoded third-from-last frame goes to the image embedder, its latent to the concat
    conditioning (no re-encode) -- both are written into `value_dict`, whose other entries are the round's -- and the last three latents are
    carried over as conditioning frames. Returns the new window; its frames [CARRY:] are the round's contribution. The two halves
    (next_round_inputs: what depends on the window only; next_round_condition: what depends on the action too) are vista_amd.plan's as well,
    which scores several actions from one window."""
    value_dict["cond_frames_without_noise"], value_dict["cond_frames"], seeded = next_round_inputs(model, sample, num_frames, device)
    c, uc = next_round_condition(model, value_dict, num_frames, get_condition, force_uc_zero_embeddings, device)
    return sampler(denoiser, noise_fn(seeded), cond=c, uc=uc, cond_frame=seeded, cond_mask=carry_mask)


@torch.no_grad()
def do_sample(images, model, sampler, value_dict, num_rounds, num_frames, force_uc_zero_embeddings=None, initial_cond_indices=None,
              device="cuda", get_condition=None, noise_fn=None, fused=True):
    """-> (samples in [0,1], samples_z, images). Same contract as the reference's do_sample; two optional hooks on top:
    `get_condition(model, value_dict, num_frames, force_uc_zero_embeddings, device) -> (c, uc)` and `noise_fn(like)`
    (default torch.randn_like) so a test can feed the very noise a CPU reference run drew. `fused`: hand the sampler a
    FusedDenoiser (its one-pass prepare/combine/Euler kernels) instead of the reference's opaque closure; same arithmetic.
    The round bodies (first_round / next_round) are shared with vista_amd.drive.DriveSession, which holds a rollout open between rounds."""
    initial_cond_indices = [0] if initial_cond_indices is None else initial_cond_indices
    force_uc_zero_embeddings = [] if force_uc_zero_embeddings is None else force_uc_zero_embeddings
    get_condition = get_condition or getattr(model, "condition_fn", None)
    if get_condition is None:
        raise ValueError("do_sample: no conditioner -- build the pipeline with conditioner=GeneralConditioner(...) or pass get_condition=")
    noise_fn = noise_fn or torch.randn_like
    carry = CARRY
    fresh = num_frames - carry                 # new frames every later round contributes
    denoiser = rollout_denoiser(model, fused)

    with model.ema_scope("Sampling"):
        c, uc = get_condition(model, value_dict, num_frames, force_uc_zero_embeddings, device)
        z = model.encode_first_stage(images)
        samples_z = torch.zeros((num_rounds * fresh + carry,) + tuple(z.shape[1:]), device=device, dtype=z.dtype)
        first_mask, carry_mask = rollout_masks(num_frames, initial_cond_indices, device)

        sample = first_round(sampler, denoiser, c, uc, z, first_mask, noise_fn)
        samples_z[:num_frames] = sample

        for n in range(1, num_rounds):
            sample = next_round(model, sampler, denoiser, value_dict, sample, num_frames, carry_mask, get_condition, force_uc_zero_embeddings,
                                device, noise_fn)
            lo = n * fresh + carry
            samples_z[lo:lo + fresh] = sample[carry:]

        samples_x = model.decode_first_stage(samples_z)
    samples = torch.clamp((samples_x + 1.0) / 2.0, min=0.0, max=1.0)
    return samples, samples_z, images


# the rest of the reference's sample_utils.py / sample.py helpers (model and sampler factories, dataset lookup, picture I/O) live in
# vista_amd/pipeline.py; they are exported here because this is where the reference's users look for them
from .pipeline import (DATASET2SOURCES, SAMPLERS, VERSION2SPECS, check_sizes, eval_clip, eval_motion, get_discretization, get_guider, get_sample, get_sampler,  # noqa: E402,F401
                       init_embedder_options, init_model, init_sampling, load_img, load_img_seq, load_model_from_config,
                       perform_save_locally, png_format, read_video_frames, sampler_name, save_video, scene_ranks, video_format)
