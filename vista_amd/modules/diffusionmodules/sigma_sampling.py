"""Which noise level a clip is scored (in training: trained) at. The class names, constructor kwargs, defaults and `target:` strings are the
reference's (tests/golden/loss_api.json pins them); the code is this project's.

Both samplers make ONE draw per clip from torch's CPU generator and hand every frame of the clip that value: `sampler(n_samples)` returns
n_samples values for n_samples // num_frames clips. `rand=` replaces the per-frame values; the generator is still advanced by the draw, so a
run that passes `rand` and one that does not leave the generator in the same state (the reference behaves so, and a seeded comparison depends
on it)."""
import torch

from ...util import instantiate_from_config


def _per_clip(draw, n_samples, num_frames, rand):
    """draw(clips) -> one value per clip; -> `rand` if given, else each clip's value repeated over its num_frames frames. The draw is made either way."""
    per_frame = draw(n_samples // num_frames).repeat_interleave(num_frames)
    return per_frame if rand is None else rand


class EDMSampling:
    """sigma = exp(p_mean + p_std * z), z ~ N(0, 1): the log-normal of Karras et al."""

    def __init__(self, p_mean=-1.2, p_std=1.2, num_frames=25):
        self.p_mean, self.p_std, self.num_frames = p_mean, p_std, num_frames

    def __call__(self, n_samples, rand=None):
        z = _per_clip(lambda clips: torch.randn((clips,)), n_samples, self.num_frames, rand)
        return torch.exp(self.p_mean + self.p_std * z)


class DiscreteSampling:
    """A uniformly drawn entry of a discretization's schedule of num_idx noise levels (`sigmas`; ascending with the default flip=True)."""

    def __init__(self, discretization_config, num_idx, do_append_zero=False, flip=True, num_frames=25):
        schedule = instantiate_from_config(discretization_config)
        self.sigmas = schedule(num_idx, do_append_zero=do_append_zero, flip=flip)
        self.num_idx, self.num_frames = num_idx, num_frames

    def __call__(self, n_samples, rand=None):
        """`rand`, where given, holds schedule indices, not normal deviates."""
        index = _per_clip(lambda clips: torch.randint(0, self.num_idx, (clips,)), n_samples, self.num_frames, rand)
        return self.sigmas[index]
