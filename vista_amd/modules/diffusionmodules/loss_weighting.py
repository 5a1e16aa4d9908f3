"""w(sigma), the weight of a noise level in the denoising loss. The class names, constructor kwargs, defaults and `target:` strings are the
reference's (tests/golden/loss_api.json pins them), so its `loss_weighting_config` blocks resolve here; the code is this project's.

All four are one family: with a data scale d, the EDM weight is (sigma^2 + d^2) / (sigma d)^2 -- the inverse of c_out^2 of the EDM
preconditioning, which makes the effective loss on the network output uniform over noise levels. d = 1 is the v-prediction weight; the two
degenerate members are 1 (no weighting) and sigma^-2 (the eps-prediction weight, the d -> infinity limit). Host arithmetic on one value per image,
evaluated in the dtype of the sigmas handed in; the front door (vista_amd/denoise_loss.py) applies the result in float64."""
import torch


class _Weighting:
    """A callable sigma -> w(sigma), elementwise, same shape / dtype / device as its argument."""

    def weight(self, sigma):
        raise NotImplementedError

    def __call__(self, sigma):
        return self.weight(sigma)


class UnitWeighting(_Weighting):
    def weight(self, sigma):
        return torch.ones_like(sigma)


class EDMWeighting(_Weighting):
    def __init__(self, sigma_data=0.5):
        self.sigma_data = sigma_data

    def weight(self, sigma):
        d = self.sigma_data
        total_variance = sigma.square() + d * d
        return total_variance / (sigma * d).square()


class VWeighting(EDMWeighting):
    def __init__(self):
        EDMWeighting.__init__(self, sigma_data=1.0)


class EpsWeighting(_Weighting):
    def weight(self, sigma):
        return torch.pow(sigma, -2.0)
