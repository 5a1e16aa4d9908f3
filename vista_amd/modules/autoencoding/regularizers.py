"""`vwm.modules.autoencoding.regularizers.DiagonalGaussianRegularizer` (configs/inference/vista.yaml:152-153) resolves here."""
from ...models.autoencoder import DiagonalGaussianRegularizer  # noqa: F401
