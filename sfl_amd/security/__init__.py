from .aggregation import Aggregator, SecureAggregator, SparsePlainAggregator  # noqa: F401
