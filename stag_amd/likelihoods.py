"""Observation models on top of the last layer's probabilities
(reference: stag/likelihoods.py:1-38; dense epilogue, no graph work)."""
import abc
import os

import torch


VALIDATE_ON_DEVICE = os.environ.get("STAG_VALIDATE_ARGS", "0") == "1"


def _validate(feat):
    """torch's argument validation reads a reduction of the probabilities back to the host — a synchronisation per
    Monte-Carlo sample and not capturable in a hipGraph: off for device tensors (None = torch's default elsewhere).
    Unlike the reference, invalid probabilities (negative, NaN) on the device therefore do not raise here; set
    `stag_amd.likelihoods.VALIDATE_ON_DEVICE = True` (or STAG_VALIDATE_ARGS=1) to get torch's check back while
    debugging."""
    return (None if VALIDATE_ON_DEVICE else False) if feat.is_cuda else None


class Likelihood(torch.nn.Module, abc.ABC):
    def __init__(self, distribution):
        super().__init__()
        self.distribution = distribution

    @abc.abstractmethod
    def condition(self, feat):
        raise NotImplementedError

    def log_prob(self, feat, y):
        return self.condition(feat).log_prob(y)

    def mean_nll(self, feat, y, mask=None):
        """(-log_prob(feat, y))[mask].mean(), the likelihood term of the objective (stag/models.py:73-76), composed from
        this object's own log_prob: a subclass that overrides log_prob or condition keeps its meaning."""
        from .models import _masked_mean
        return _masked_mean(-self.log_prob(feat, y), mask)


def _fused_mean_nll(likelihood, feat, y, mask):
    """The masked mean NLL of one of the two shipped classes: one fused pass each way where ops.nll_why_not has no
    objection (stag_nll_categorical_fwd / _bwd, stag_nll_bernoulli_fwd / _bwd), else the composed expression."""
    from . import ops
    if ops.nll_why_not(likelihood, feat, y, mask) is None:
        return ops.nll_mean(likelihood, feat, y, mask)
    return Likelihood.mean_nll(likelihood, feat, y, mask)


class CategoricalLikelihood(Likelihood):
    def __init__(self):
        super().__init__(torch.distributions.Categorical)

    def condition(self, feat):
        return self.distribution(probs=feat, validate_args=_validate(feat))

    def mean_nll(self, feat, y, mask=None):
        return _fused_mean_nll(self, feat, y, mask)


class BernoulliLikelihood(Likelihood):
    def __init__(self):
        super().__init__(torch.distributions.Bernoulli)

    def condition(self, feat):
        return self.distribution(probs=feat, validate_args=_validate(feat))

    def mean_nll(self, feat, y, mask=None):
        return _fused_mean_nll(self, feat, y, mask)
