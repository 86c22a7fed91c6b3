from .crf_as_rnn import CRFRNN  # noqa: F401

__all__ = ["CRFRNN"]
