"""`neurosis.modules.autoencoding.regularizers` on MI355X: what sits between an autoencoder's encoder and decoder.
DiagonalGaussianRegularizer (the KL-VAE's) lives with the engine in neurosis_amd.models.autoencoder and is re-exported here; the
vector quantizers are in .quantize, over the code-search / statistics / gather kernels of csrc/vq.hip."""
from ....models.autoencoder import DiagonalGaussianRegularizer
from .base import AbstractRegularizer, IdentityRegularizer, measure_perplexity
from .quantize import AbstractQuantizer, EmbeddingEMA, EMAVectorQuantizer, VectorQuantizer

__all__ = ["AbstractRegularizer", "IdentityRegularizer", "measure_perplexity", "DiagonalGaussianRegularizer", "AbstractQuantizer",
           "VectorQuantizer", "EmbeddingEMA", "EMAVectorQuantizer"]
