"""`neurosis.modules.autoencoding.regularizers.base`: the regularizer interface and the codebook-usage measure."""
from __future__ import annotations

from abc import abstractmethod
from typing import Any, Tuple

import torch
from torch import Tensor, nn


class AbstractRegularizer(nn.Module):
    def __init__(self):
        super().__init__()

    def forward(self, z: Tensor) -> Tuple[Tensor, dict]:
        raise NotImplementedError(f"{type(self).__name__} defines no forward")

    @abstractmethod
    def get_trainable_parameters(self) -> Any:
        raise NotImplementedError(f"{type(self).__name__} does not say which parameters it trains")


class IdentityRegularizer(AbstractRegularizer):
    loss_key = None

    def forward(self, z: Tensor) -> Tuple[Tensor, dict]:
        return z, dict()

    def regularize(self, z: Tensor, noise=None):
        """the engine's protocol: (z, log, bwd) with bwd(dz, weight) -> dz"""
        return z, dict(), lambda dz, weight=0.0: dz

    def get_trainable_parameters(self) -> Any:
        yield from ()


def perplexity_from_counts(count: Tensor) -> Tuple[Tensor, Tensor]:
    """(perplexity, cluster_use) from how often each centroid was chosen: exp(-sum p log(p + 1e-10)) with p = count / N, and the
    number of centroids in use.  count / N is what the mean of the reference's one-hot matrix gives (both exact up to the division)."""
    avg_probs = count.to(torch.float32) / count.sum().to(torch.float32)
    perplexity = (-(avg_probs * torch.log(avg_probs + 1e-10)).sum()).exp()
    return perplexity, torch.sum(avg_probs > 0)


def measure_perplexity(predicted_indices: Tensor, num_centroids: int) -> Tuple[Tensor, Tensor]:
    """eval cluster perplexity: when perplexity == num_embeddings all clusters are used exactly equally.  The reference builds the
    [N, num_centroids] one-hot matrix and averages it; a bincount holds the same information in num_centroids integers."""
    return perplexity_from_counts(torch.bincount(predicted_indices.reshape(-1), minlength=num_centroids))
