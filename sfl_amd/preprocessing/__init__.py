"""The reference's ``sfl.preprocessing``: what runs on the data before a model does."""
from . import binning
