from .boost import FeatureHistogram

__all__ = ["FeatureHistogram"]
