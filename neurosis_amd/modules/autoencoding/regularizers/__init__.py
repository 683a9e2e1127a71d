"""`neurosis.modules.autoencoding.regularizers` on MI355X: what sits between an autoencoder's encoder and decoder.
DiagonalGaussianRegularizer (the KL-VAE's) lives with the engine in neurosis_amd.models.autoencoder and is re-exported here; the
vector quantizers are in .quantize, over the code-search / statistics / gather kernels of csrc/vq.hip; GumbelQuantizer is in .gumbel, over the
Gumbel-softmax kernels of csrc/gumbel.hip."""
from ....models.autoencoder import DiagonalGaussianRegularizer
from .base import AbstractRegularizer, IdentityRegularizer, measure_perplexity
from .quantize import AbstractQuantizer, EmbeddingEMA, EMAVectorQuantizer, VectorQuantizer
from .gumbel import GumbelQuantizer

__all__ = ["AbstractRegularizer", "IdentityRegularizer", "measure_perplexity", "DiagonalGaussianRegularizer", "AbstractQuantizer",
           "VectorQuantizer", "EmbeddingEMA", "EMAVectorQuantizer", "GumbelQuantizer"]
