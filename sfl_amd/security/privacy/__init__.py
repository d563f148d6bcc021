"""Differential-privacy pre-step of the FL secure-aggregation path
(mirrors sfl/security/privacy)."""
from .mechanism import DPStrategyFL, GaussianModelDP, SecureGaussianModelDP  # noqa: F401
from .smp import SMPMask, smp_step  # noqa: F401
