"""The reference's ``sfl.preprocessing.binning`` on the GPU: federated quantile split points."""
from .homo_binning import HomoBinning
