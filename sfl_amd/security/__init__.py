from .aggregation import Aggregator, FlameAggregator, SecureAggregator, SparsePlainAggregator  # noqa: F401
