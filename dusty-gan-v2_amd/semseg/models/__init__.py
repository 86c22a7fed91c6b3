from .crf_as_rnn import CRFRNN  # noqa: F401
from .knn import kNN2d  # noqa: F401
from .loss import FocalLoss, MaskedSegLoss  # noqa: F401
from .squeezeseg_v1 import SqueezeSegV1  # noqa: F401
from .squeezeseg_v2 import SqueezeSegV2  # noqa: F401
from .syncbn import SyncBatchNorm2d, convert_sync_batchnorm  # noqa: F401

__all__ = ["CRFRNN", "kNN2d", "FocalLoss", "MaskedSegLoss", "SqueezeSegV1", "SqueezeSegV2", "SyncBatchNorm2d",
           "convert_sync_batchnorm"]
