"""Reward estimation around the sampler (reference: reward_utils.py:284-341, `do_sample`; driver reward.py:225-250):
`ensemble_size` sampling runs from the same conditioning with fresh noise; the reward is exp(-mean over all latent elements
of the unbiased ensemble variance) -- low disagreement between the imagined futures = high reward.

Pure re-use of the hot path: the ensemble members run through the same sampler/denoiser objects;
only the variance reduction is new (one fixed-order HIP reduction, vk_ensemble_variance_sum). `model` is duck-typed like in
vista_amd.sample_utils (VistaPipeline or the reference engine); `get_condition` / `noise_fn` are the same optional hooks.

`estimate` is the driver's form of the same computation (vista_amd/reward.py): several candidate actions scored on one scene under common
random numbers, the variance kept per frame and per latent pixel (vk_ensemble_frame_stats), and the members optionally spread over ranks.
"""
import dataclasses
import math
from typing import Optional

import torch

from . import ops
from .modules.diffusionmodules.denoiser import Denoiser
from .modules.diffusionmodules.sampling import FusedDenoiser


@torch.no_grad()
def do_sample(images, model, sampler, value_dict, num_frames, ensemble_size: int = 5, force_uc_zero_embeddings=None,
              initial_cond_indices=None, device="cuda", get_condition=None, noise_fn=None, fused=True):
    """-> (images, reward) with reward a 0-dim CPU tensor, like the reference."""
    if ensemble_size < 2:
        raise ValueError("reward estimation needs at least two ensemble members (unbiased variance)")
    initial_cond_indices = [0] if initial_cond_indices is None else initial_cond_indices
    force_uc_zero_embeddings = [] if force_uc_zero_embeddings is None else force_uc_zero_embeddings
    get_condition = get_condition or getattr(model, "condition_fn", None)
    if get_condition is None:
        raise ValueError("do_sample: no conditioner -- pass get_condition=")
    noise_fn = noise_fn or torch.randn_like

    def denoiser(x, sigma, cond, cond_mask):
        return model.denoiser(model.model, x, sigma, cond, cond_mask)
    if fused and isinstance(model.denoiser, Denoiser):
        denoiser = FusedDenoiser(model.denoiser, model.model)

    with model.ema_scope("Sampling"):
        z = model.encode_first_stage(images)
        cond_mask = torch.zeros(num_frames, device=device)
        cond_mask[initial_cond_indices] = 1
        c, uc = get_condition(model, value_dict, num_frames, force_uc_zero_embeddings, device)
        members = []
        for _ in range(ensemble_size):
            sample = sampler(denoiser, noise_fn(z), cond=c, uc=uc, cond_frame=z, cond_mask=cond_mask)
            sample[0] = z[0]
            members.append(sample.float())
        stacked = torch.stack(members).contiguous()                     # (E, T, 4, h, w)
        var_sum = ops.ensemble_variance_sum(stacked)                    # sum over elements of sum_e (x_e - mean_e)^2 / (E - 1)
        reward = torch.tensor(math.exp(-var_sum / stacked[0].numel()))  # exp(-variance.mean())
    return images, reward


@dataclasses.dataclass
class RewardReport:
    """What one candidate action's ensemble says. `reward` is the reference's exp(-variance.mean()) as a 0-dim float64 CPU tensor;
    `frame_variance` (T,) float64 on the CPU is the mean variance of every frame's latent elements (frame 0 is the conditioning frame: exactly
    0), `frame_reward` its exp(-.); `map` (T, h, w) float32 on the GPU is the variance averaged over the latent channels, or None."""
    reward: torch.Tensor
    mean_variance: float
    frame_variance: torch.Tensor
    frame_reward: torch.Tensor
    map: Optional[torch.Tensor] = None


def member_slots(ensemble_size, world):
    """Which ensemble members each rank of an ensemble-parallel run samples: member e belongs to rank e % world.
    -> a list of `world` lists of member indices (ascending); every member appears exactly once."""
    if ensemble_size < 2:
        raise ValueError("reward estimation needs at least two ensemble members (unbiased variance)")
    if world < 1:
        raise ValueError(f"member_slots: world must be at least 1, got {world}")
    if world > ensemble_size:
        raise ValueError(f"world {world} > ensemble_size {ensemble_size}: every rank of an ensemble-parallel run needs at least one member")
    return [list(range(rank, ensemble_size, world)) for rank in range(world)]


@torch.no_grad()
def estimate(images, model, sampler, value_dicts, num_frames, ensemble_size: int = 5, force_uc_zero_embeddings=None,
             initial_cond_indices=None, device="cuda", get_condition=None, noise_fn=None, fused=True, want_map=True, members=None, comm=None):
    """-> one RewardReport per candidate. `value_dicts`: one value dict per candidate action (a single dict = one candidate). The first stage
    encodes once, the conditioner runs once per candidate, and the `ensemble_size` noise tensors are drawn ONCE, in member order, and reused for
    every candidate (common random numbers: the difference between two candidates' rewards is not noise from different draws). For one
    candidate and the same `noise_fn` the reward is do_sample's up to the order of one fp64 sum.
    `members=(rank, world)`, `comm` (all_reduce_sum, as the groups of vista_amd/parallel.py offer it): rank r samples the members of
    member_slots(ensemble_size, world)[r] only. Every rank still draws all the noises in order (its random stream stays the single-process
    one), writes its members into a zero-filled (E, T, C, h, w) buffer, and one all_reduce per candidate completes the buffer everywhere
    (adding zeros is exact): every rank returns the same reports."""
    if isinstance(value_dicts, dict):
        value_dicts = [value_dicts]
    rank, world = (0, 1) if members is None else members
    slots = member_slots(ensemble_size, world)
    if not 0 <= rank < world:
        raise ValueError(f"members=({rank}, {world}): the rank must lie in [0, world)")
    if world > 1 and comm is None:
        raise ValueError("estimate: members over several ranks need comm= (a communicator with all_reduce_sum)")
    initial_cond_indices = [0] if initial_cond_indices is None else initial_cond_indices
    force_uc_zero_embeddings = [] if force_uc_zero_embeddings is None else force_uc_zero_embeddings
    get_condition = get_condition or getattr(model, "condition_fn", None)
    if get_condition is None:
        raise ValueError("estimate: no conditioner -- pass get_condition=")
    noise_fn = noise_fn or torch.randn_like

    def denoiser(x, sigma, cond, cond_mask):
        return model.denoiser(model.model, x, sigma, cond, cond_mask)
    if fused and isinstance(model.denoiser, Denoiser):
        denoiser = FusedDenoiser(model.denoiser, model.model)

    reports = []
    with model.ema_scope("Sampling"):
        z = model.encode_first_stage(images)
        cond_mask = torch.zeros(num_frames, device=device)
        cond_mask[initial_cond_indices] = 1
        # do_sample's order -- encode, condition, then the members' noise -- so that one candidate sees do_sample's random stream
        conditions = [get_condition(model, value_dict, num_frames, force_uc_zero_embeddings, device) for value_dict in value_dicts]
        noises = {}
        for e in range(ensemble_size):
            noise = noise_fn(z)          # every rank draws every member's noise, in order ...
            if e in slots[rank]:
                noises[e] = noise        # ... and keeps its own
        for c, uc in conditions:
            stacked = torch.zeros((ensemble_size,) + tuple(z.shape), dtype=torch.float32, device=z.device)   # (E, T, 4, h, w)
            for e in slots[rank]:
                # (the sampler scales its input in place: every candidate gets a copy of the member's noise)
                sample = sampler(denoiser, noises[e].clone(), cond=c, uc=uc, cond_frame=z, cond_mask=cond_mask)
                sample[0] = z[0]
                stacked[e] = sample
            if world > 1:
                comm.all_reduce_sum(stacked)
            frame_sum, fmap = ops.ensemble_frame_stats(stacked, want_map=want_map)
            # Frame 0 is z[0] in every member (the assignment above), so its variance is 0 by construction. The fp32 mean of E equal values is
            # not always that value ((x + x + x) / 3 can land one ulp beside x), which leaves a residue of ~1e-17 in the kernel's sum: the
            # report states the exact value instead of the residue (a change of ~1e-16 relative in the mean, far inside the summation-order bound).
            frame_sum[0] = 0.0
            if fmap is not None:
                fmap[0].zero_()
            frame_sum = frame_sum.cpu()
            per_frame = stacked[0, 0].numel()
            frame_variance = frame_sum / per_frame
            mean_variance = float(frame_sum.sum()) / (per_frame * frame_sum.numel())
            reports.append(RewardReport(reward=torch.tensor(math.exp(-mean_variance), dtype=torch.float64), mean_variance=mean_variance,
                                        frame_variance=frame_variance, frame_reward=torch.exp(-frame_variance), map=fmap))
    return reports
