"""The denoising loss of a checkpoint on real latents, forward only (reference: vwm/modules/diffusionmodules/loss.py, StandardDiffusionLoss).

Same class name, constructor, defaults and `target:` string as the reference, so its `loss_fn_config` blocks instantiate unchanged. Everything
here runs under torch.no_grad(): this is a measurement. Training -- gradients, optimisers, EMA, the loop -- is NOT built, and nothing
returned here carries a graph.

The arithmetic is three HIP entry points (csrc/loss.hip): the noising of the input (vk_loss_noise_input, bit for bit the reference's fp32
expression), the Fourier high-pass of predict - target (vk_fourier_highpass) and the per-frame sums (vk_loss_stats, fp64, fixed order). The
per-frame loss weight w(sigma) is applied on the host in float64, so a report can carry weighted and unweighted figures from one set of sums;
`get_loss` assembles the reference's totals from them and returns float64 tensors on the host.
"""
import random
from typing import Dict

import torch
import torch.nn as nn

from ... import ops
from ...util import instantiate_from_config
from .util import fourier_keep_mask_on


class StandardDiffusionLoss(nn.Module):
    """Constructor arguments (the reference's names and defaults; tests/golden/loss_api.json pins them):
      sigma_sampler_config, loss_weighting_config   `target:` blocks of a sigma sampler and a weighting (sigma_sampling.py, loss_weighting.py)
      loss_type                                     "l2" (squares) or "l1" (absolute values)
      use_additional_loss, additional_loss_weight   the dynamics weight and the Fourier high-pass term, and the latter's factor
      offset_noise_level                            > 0: noise + level * N(0, 1) per (image, channel)
      num_frames                                    frames per clip: images b * num_frames .. (b + 1) * num_frames - 1 are clip b
      replace_cond_frames, cond_frames_choices      keep some frames of every clip clean and out of the loss; the index lists to choose from"""

    def __init__(self, sigma_sampler_config, loss_weighting_config, loss_type="l2", use_additional_loss=False, offset_noise_level=0.0,
                 additional_loss_weight=0.0, num_frames=25, replace_cond_frames=False, cond_frames_choices=None):
        super().__init__()
        if loss_type not in ("l2", "l1"):
            raise ValueError(f"loss_type {loss_type!r}: 'l2' or 'l1'")
        self.sigma_sampler, self.loss_weighting = (instantiate_from_config(c) for c in (sigma_sampler_config, loss_weighting_config))
        self.loss_type, self.num_frames = loss_type, num_frames
        self.use_additional_loss, self.additional_loss_weight = use_additional_loss, additional_loss_weight
        self.offset_noise_level = offset_noise_level
        self.replace_cond_frames, self.cond_frames_choices = replace_cond_frames, cond_frames_choices

    @torch.no_grad()
    def get_noised_input(self, sigmas_bc: torch.Tensor, noise: torch.Tensor, input: torch.Tensor) -> torch.Tensor:
        """input + noise * sigmas_bc, sigmas_bc one value per image (any shape with n elements)."""
        return ops.loss_noise_input(input.float().contiguous(), noise.float().contiguous(), sigmas_bc.reshape(-1).float().contiguous())

    @torch.no_grad()
    def forward(self, network: nn.Module, denoiser, conditioner, input: torch.Tensor, batch: Dict) -> torch.Tensor:
        cond = conditioner(batch)
        return self._forward(network, denoiser, cond, input)

    def draw_cond_mask(self, n):
        """(n,) of 0 / 1 on the host: every clip gets one of cond_frames_choices as its conditioning frames, list k with probability proportional
        to 2^k (later lists, which hold more frames, are the likelier ones). One random.choices call per clip, in clip order: Python's generator
        is consumed as the reference consumes it, so a seeded run picks the same lists."""
        lists = self.cond_frames_choices
        if not lists or max(len(frames) for frames in lists) >= self.num_frames:
            raise ValueError(f"cond_frames_choices {lists}: needs at least one list, each shorter than a clip of {self.num_frames} frames")
        odds = [1 << k for k in range(len(lists))]
        clips = n // self.num_frames
        picks = [random.choices(range(len(lists)), weights=odds, k=1)[0] for _ in range(clips)]
        mask = torch.zeros(clips, self.num_frames)
        for clip, k in enumerate(picks):
            mask[clip, lists[k]] = 1.0
        return mask.reshape(-1)

    @torch.no_grad()
    def _forward(self, network: nn.Module, denoiser, cond: Dict, input: torch.Tensor, *, sigmas=None, cond_mask=None, noise=None, offset=None,
                 return_sums=False):
        """The reference's _forward, forward only. Draws, in the reference's order: the sigma sampler (CPU generator), random.choices per clip
        (only with replace_cond_frames), randn_like(input), the offset noise (n, C) (only with offset_noise_level > 0). An explicit `sigmas`,
        `cond_mask`, `noise` or `offset` replaces that draw (and the draw is then not made), in the spirit of do_sample(noise_fn=).
        return_sums: also return the per-frame sums (n, 3) float64 and w (n,) float64, both on the host."""
        input = input.float().contiguous()
        n, dev = input.shape[0], input.device
        sigmas = (self.sigma_sampler(n) if sigmas is None else sigmas).to(device=dev, dtype=torch.float32).contiguous()
        if self.replace_cond_frames:
            cond_mask = (self.draw_cond_mask(n) if cond_mask is None else cond_mask).to(device=dev, dtype=torch.float32).contiguous()
        else:
            cond_mask = torch.zeros_like(sigmas)
        noise = (torch.randn_like(input) if noise is None else noise.to(device=dev, dtype=torch.float32)).contiguous()
        if self.offset_noise_level > 0.0:   # the entire channel is shifted together
            offset = (torch.randn((n, input.shape[1]), device=dev) if offset is None else offset.to(device=dev, dtype=torch.float32)).contiguous()
        else:
            offset = None
        noised_input = ops.loss_noise_input(input, noise, sigmas, cond_mask if self.replace_cond_frames else None, offset,
                                            self.offset_noise_level)
        model_output = denoiser(network, noised_input, sigmas, cond, cond_mask)
        w = self.loss_weighting(sigmas)
        return self._loss_from_output(model_output, input, w, cond_mask if self.replace_cond_frames else None, return_sums)

    @torch.no_grad()
    def get_loss(self, predict, target, w):
        """The reference's get_loss(predict, target, w): w one weight per image (any shape with n elements). The per-image vector without
        use_additional_loss, the scalar with it; float64, on the host."""
        return self._loss_from_output(predict, target, w, None, False)

    def loss_sums(self, model_output, target, cond_mask=None):
        """(n, 3) float64 on the GPU: per frame S0 = sum e, S1 = sum e * aux_w, S2 = sum |HF(predict - target)|^p (include/vista_hip.h), with the
        replace_cond_frames blend predict = output * (1 - m) + target * m fused in where cond_mask is given. S1 = S0 and S2 = 0 without
        use_additional_loss."""
        model_output, target = model_output.float().contiguous(), target.float().contiguous()
        hf = None
        if self.use_additional_loss:
            H, W = target.shape[-2:]
            hf = ops.fourier_highpass(model_output, fourier_keep_mask_on(target.device, H, W), 0.0, b=target, cond_mask=cond_mask)
        return ops.loss_stats(model_output, target, self.num_frames if self.use_additional_loss else 1, cond_mask=cond_mask, hf=hf,
                              l1=self.loss_type == "l1")

    def _loss_from_output(self, model_output, target, w, cond_mask, return_sums):
        sums = self.loss_sums(model_output, target, cond_mask).cpu()   # (the copy ends the stage)
        w64 = w.reshape(-1).to(device="cpu", dtype=torch.float64)
        loss = self.assemble(sums, w64, target[0].numel())
        return (loss, sums, w64) if return_sums else loss

    def assemble(self, sums, w64, per_image):
        """sums (n, 3) and w (n,) float64 on the host -> the reference's total: w_i S0_i / (C h w) per image, or with the additional terms
        mean_i[w_i S1_i / (C h w)] + additional_loss_weight * mean_i[w_i S2_i / (C h w)]."""
        if not self.use_additional_loss:
            return w64 * sums[:, 0] / per_image
        return (w64 * sums[:, 1] / per_image).mean() + self.additional_loss_weight * (w64 * sums[:, 2] / per_image).mean()
