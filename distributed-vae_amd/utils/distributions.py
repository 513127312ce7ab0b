"""Count distributions on the device: the counterpart of the reference's ``mmidas/utils/distributions.py`` (the scVI
likelihoods and distribution classes), on the kernels of csrc/countdist.hip.

GPU float32 tensors only (a CPU tensor raises ``NativeError``); every value behind the float32 inputs is computed in fp64.
What differs from the reference, on purpose:

* ``softplus`` has no switch to the identity above 20, and the mixture's logsumexp is taken about its maximum;
* ``log_zinb_positive`` evaluates only the branch that ``x < eps`` or ``x > eps`` selects -- the reference multiplies the
  other branch by an exact 0, which differs only where that other branch is not finite; ``x == eps`` gives 0 as there;
* the three functions take ``reduce="sums"`` and then return ``{"cell": float64 [N], "gene": float64 [D]}`` without ever
  writing the N x D terms;
* ``sample`` takes ``seed`` and ``offset``: the draws come from the in-kernel Philox stream (a function of seed, offset and
  the element's index alone), not from torch's generator -- ``seed=None`` draws the seed from torch's generator, so that
  ``torch.manual_seed`` reproduces a run;
* ``ZeroInflatedNegativeBinomial`` also accepts ``zi_probs``; ``validate_args`` only exists.
"""
from typing import Optional, Tuple, Union

import torch

from .. import _native as N

__all__ = ["log_zinb_positive", "log_nb_positive", "log_mixture_nb", "NegativeBinomial", "ZeroInflatedNegativeBinomial",
           "NegativeBinomialMixture"]


def _as_2d(what: str, x: torch.Tensor):
    """(x as float32 [N, D], the shape to give back)"""
    if not isinstance(x, torch.Tensor):
        raise TypeError(f"{what}: expected a tensor, got {type(x).__name__}")
    N._need_cuda(what, x)
    shape = tuple(x.shape)
    x = x.float()
    return (x.reshape(1, -1) if x.dim() < 2 else x.reshape(-1, shape[-1])), shape


def _like(what: str, name: str, t: torch.Tensor, x2: torch.Tensor, shape, vector_ok: bool = False):
    """``t`` as the kernels take it beside x2 [N, D]: float32 [N, D] (broadcast if it must be) or, for theta, [D]."""
    N._need_cuda(what, t)
    t = t.float()
    D = x2.shape[1]
    if vector_ok and t.dim() == 1 and t.shape[0] == D:
        return t
    if vector_ok and t.dim() == 2 and t.shape == (1, D) and len(shape) == 2:      # the reference's theta.view(1, D)
        return t.reshape(D)
    if tuple(t.shape) != tuple(shape):
        try:
            t = t.expand(shape)
        except RuntimeError:
            raise ValueError(f"{what}: {name} of shape {tuple(t.shape)} does not broadcast to {tuple(shape)}") from None
    return t.reshape(x2.shape)


def _logp(what, kind, x, mu, theta, pi, mu2, theta2, eps, reduce):
    if reduce not in ("none", "sums"):
        raise ValueError(f"{what}: reduce must be 'none' or 'sums'; got {reduce!r}")
    x2, shape = _as_2d(what, x)
    args = {"mu": _like(what, "mu", mu, x2, shape), "theta": _like(what, "theta", theta, x2, shape, True)}
    if pi is not None:
        args["pi"] = _like(what, "pi", pi, x2, shape)
    if mu2 is not None:
        args["mu2"] = _like(what, "mu_2", mu2, x2, shape)
    if theta2 is not None:
        args["theta2"] = _like(what, "theta_2", theta2, x2, shape, True)
    sums = reduce == "sums"
    terms, cell, gene = N.count_logp(kind, x2, eps=eps, return_terms=not sums, return_sums=sums, **args)
    return {"cell": cell, "gene": gene} if sums else terms.reshape(shape)


def log_zinb_positive(x: torch.Tensor, mu: torch.Tensor, theta: torch.Tensor, pi: torch.Tensor, eps=1e-8, reduce: str = "none"):
    """Log likelihood of ``x`` under a zero-inflated negative binomial: ``mu`` the mean, ``theta`` the inverse dispersion
    ([D], shared by all cells, or minibatch x vars), ``pi`` the logit of the dropout.  float32 device tensor of x's shape, or
    the per-cell / per-gene sums with ``reduce="sums"``."""
    return _logp("log_zinb_positive", "zinb", x, mu, theta, pi, None, None, eps, reduce)


def log_nb_positive(x: torch.Tensor, mu: torch.Tensor, theta: torch.Tensor, eps=1e-8, reduce: str = "none"):
    """Log likelihood of ``x`` under a negative binomial with mean ``mu`` and inverse dispersion ``theta``."""
    return _logp("log_nb_positive", "nb", x, mu, theta, None, None, None, eps, reduce)


def log_mixture_nb(x: torch.Tensor, mu_1: torch.Tensor, mu_2: torch.Tensor, theta_1: torch.Tensor, theta_2: Optional[torch.Tensor],
                   pi_logits: torch.Tensor, eps=1e-8, reduce: str = "none"):
    """Log likelihood of ``x`` under a mixture of two negative binomials; ``pi_logits`` is the logit of belonging to the first
    component, ``theta_2=None`` shares ``theta_1``."""
    return _logp("log_mixture_nb", "mixture", x, mu_1, theta_1, pi_logits, mu_2, theta_2, eps, reduce)


def _convert_mean_disp_to_counts_logits(mu, theta, eps=1e-6):
    """NB parameterisations: (mu, theta) -> (total_count, logits) = (theta, log(mu + eps) - log(theta + eps))."""
    if not (mu is None) == (theta is None):
        raise ValueError("If using the mu/theta NB parameterization, both parameters must be specified")
    return theta, (mu + eps).log() - (theta + eps).log()


def _convert_counts_logits_to_mean_disp(total_count, logits):
    """NB parameterisations: (total_count, logits) -> (mu, theta) = (exp(logits) total_count, total_count)."""
    return logits.exp() * total_count, total_count


def _seed(seed) -> int:
    if seed is None:
        return int(torch.randint(0, 2 ** 62, (1,)).item())
    return int(seed)


def _sample(what, mu, theta, zi, zi_kind, sample_shape, seed, offset):
    """sample_shape + batch_shape draws: draw j of the sample dimension takes the rows j * rows .. of the logical matrix."""
    n_rep = 1
    for v in tuple(sample_shape):
        n_rep *= int(v)
    mu2, shape = _as_2d(what, mu)
    th2 = _like(what, "theta", theta, mu2, shape, True)
    zi2 = None if zi is None else _like(what, "zi", zi, mu2, shape)
    seed = _seed(seed)
    rows = mu2.shape[0]
    out = [N.count_sample(mu2, th2, zi2, zi_kind, seed=seed, offset=offset, cell0=j * rows) for j in range(n_rep)]
    return torch.stack(out).reshape(tuple(sample_shape) + shape) if tuple(sample_shape) else out[0].reshape(shape)


class NegativeBinomial:
    """Negative binomial distribution, by (``total_count``, ``probs`` or ``logits``) or by (``mu``, ``theta``), the mean and
    the inverse dispersion.  A draw is w ~ Gamma(shape theta, rate theta / mu), then Poisson(min(w, 1e8))."""

    def __init__(self, total_count=None, probs=None, logits=None, mu=None, theta=None, validate_args: bool = False):
        self._eps = 1e-8
        if (mu is None) == (total_count is None):
            raise ValueError("Please use one of the two possible parameterizations. Refer to the documentation for more information.")
        if total_count is not None and (logits is not None or probs is not None):
            logits = logits if logits is not None else torch.log(probs) - torch.log1p(-probs)
            total_count, logits = torch.broadcast_tensors(total_count.type_as(logits), logits)
            mu, theta = _convert_counts_logits_to_mean_disp(total_count, logits)
        elif mu is None or theta is None:
            raise ValueError("total_count needs probs or logits; mu needs theta")
        else:
            mu, theta = torch.broadcast_tensors(mu, theta)
        N._need_cuda(type(self).__name__, mu, theta)
        self.mu, self.theta = mu, theta
        self._validate_args = validate_args

    @property
    def mean(self):
        return self.mu

    @property
    def variance(self):
        return self.mean + (self.mean ** 2) / self.theta

    def sample(self, sample_shape: Union[torch.Size, Tuple] = torch.Size(), seed=None, offset: int = 0) -> torch.Tensor:
        return _sample("NegativeBinomial.sample", self.mu, self.theta, None, None, sample_shape, seed, offset)

    def log_prob(self, value: torch.Tensor) -> torch.Tensor:
        return log_nb_positive(value, mu=self.mu, theta=self.theta, eps=self._eps)


class ZeroInflatedNegativeBinomial(NegativeBinomial):
    """Zero-inflated negative binomial: a NegativeBinomial whose draw is set to 0 where u <= the zero-inflation probability,
    given as ``zi_logits`` (the reference's argument) or as ``zi_probs``."""

    def __init__(self, total_count=None, probs=None, logits=None, mu=None, theta=None, zi_logits=None, zi_probs=None,
                 validate_args: bool = False):
        super().__init__(total_count=total_count, probs=probs, logits=logits, mu=mu, theta=theta, validate_args=validate_args)
        if (zi_logits is None) == (zi_probs is None):
            raise ValueError("give one of zi_logits and zi_probs")
        given = zi_logits if zi_logits is not None else zi_probs
        given, self.mu, self.theta = torch.broadcast_tensors(given, self.mu, self.theta)
        N._need_cuda(type(self).__name__, given)
        self._zi, self._zi_kind = given, "logits" if zi_logits is not None else "probs"

    @property
    def zi_logits(self) -> torch.Tensor:
        return self._zi if self._zi_kind == "logits" else torch.log(self._zi) - torch.log1p(-self._zi)

    @property
    def zi_probs(self) -> torch.Tensor:
        return self._zi if self._zi_kind == "probs" else torch.sigmoid(self._zi)

    @property
    def mean(self):
        return (1 - self.zi_probs) * self.mu

    @property
    def variance(self):
        raise NotImplementedError

    def sample(self, sample_shape: Union[torch.Size, Tuple] = torch.Size(), seed=None, offset: int = 0) -> torch.Tensor:
        return _sample("ZeroInflatedNegativeBinomial.sample", self.mu, self.theta, self._zi, self._zi_kind, sample_shape, seed, offset)

    def log_prob(self, value: torch.Tensor) -> torch.Tensor:
        return log_zinb_positive(value, self.mu, self.theta, self.zi_logits, eps=1e-08)


class NegativeBinomialMixture:
    """Mixture of two negative binomials: ``mixture_logits`` is the logit of belonging to component 1; ``theta2=None`` shares
    ``theta1``.

    ``sample`` raises NotImplementedError: there is no behaviour to mirror.  The reference's version hands (mu, theta) to its
    Gamma helper in the wrong order (so the Gamma's shape is the mean) and stores ``theta2`` as a tuple that its arithmetic
    then cannot use."""

    def __init__(self, mu1, mu2, theta1, mixture_logits, theta2=None, validate_args: bool = False):
        self.mu1, self.theta1, self.mu2, self.mixture_logits = torch.broadcast_tensors(mu1, theta1, mu2, mixture_logits)
        self.theta2 = None if theta2 is None else torch.broadcast_tensors(mu1, theta2)[1]
        N._need_cuda(type(self).__name__, self.mu1, self.theta1, self.mu2, self.mixture_logits, self.theta2)
        self._validate_args = validate_args

    @property
    def mixture_probs(self) -> torch.Tensor:
        return torch.sigmoid(self.mixture_logits)

    @property
    def mean(self):
        pi = self.mixture_probs
        return pi * self.mu1 + (1 - pi) * self.mu2

    def sample(self, sample_shape: Union[torch.Size, Tuple] = torch.Size(), seed=None, offset: int = 0) -> torch.Tensor:
        raise NotImplementedError("NegativeBinomialMixture.sample is not built: the reference's own version cannot run as written "
                                  "(see the class docstring)")

    def log_prob(self, value: torch.Tensor) -> torch.Tensor:
        return log_mixture_nb(value, self.mu1, self.mu2, self.theta1, self.theta2, self.mixture_logits, eps=1e-08)
