"""The reference's ``sfl.ml.boost`` on the GPU: the node histograms of homo_boost."""
from .feature_histogram import FeatureHistogram, scale_of

__all__ = ["FeatureHistogram", "scale_of"]
