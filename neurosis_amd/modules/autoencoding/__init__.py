"""`neurosis.modules.autoencoding` on MI355X: the loss classes an autoencoder-training config names (losses/) and what sits between
encoder and decoder (regularizers/: the Gaussian posterior and the vector quantizers)."""
from . import losses, regularizers

__all__ = ["losses", "regularizers"]
