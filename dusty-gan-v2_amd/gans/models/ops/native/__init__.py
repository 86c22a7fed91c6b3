"""Autograd-aware wrappers around the libdgv2 C ABI (include/dgv2.h).

Internal layout is channels-last: activations are contiguous [B, H, W, C] tensors in
float32 (parity mode) or bfloat16 (throughput mode, fp32 accumulate).  Parameters
stay float32 masters; weight gradients are produced in float32.

Every op that sits on the discriminator side of the R1 penalty (gans/trainer.py:419-451
of the reference) is closed under differentiation: linear ops pair a forward Function
with its transpose, convolutions form the {fwd, dgrad, wgrad} triple, bias+lrelu reuses
its masked form -- so double backward never leaves the HIP kernels.

One submodule per subject (DESIGN.md section 27 has the table).  Each imports what it uses by name from the module that defines it
and ends in a literal __all__; a module-level switch (a name read from os.environ) is never imported: other modules, tests and
scripts read and set it as <module>.<FLAG>.  Everything in a submodule's __all__ is also reachable as native.<name>.
"""
import dgv2_native as N  # noqa: F401  (native.N: the ctypes binding)
from . import (act_resample, cam, constcache, conv, crf, fire, fourier, fp8, frame, glin, inversion, kitti, knn, latent, loss, modgemm,  # noqa: F401
               modlayer, modup, optim, pointnet, render, rng, second_order, segloss, sgd, stem_tail_ada, syncbn, upsample)
from .act_resample import *  # noqa: F401,F403
from .constcache import *  # noqa: F401,F403
from .fourier import *  # noqa: F401,F403
from .glin import *  # noqa: F401,F403
from .optim import *  # noqa: F401,F403
from .modgemm import *  # noqa: F401,F403
from .fp8 import *  # noqa: F401,F403
from .conv import *  # noqa: F401,F403
from .stem_tail_ada import *  # noqa: F401,F403
from .modlayer import *  # noqa: F401,F403
from .modup import *  # noqa: F401,F403
from .second_order import *  # noqa: F401,F403
from .inversion import *  # noqa: F401,F403
from .kitti import *  # noqa: F401,F403
from .loss import *  # noqa: F401,F403
from .rng import *  # noqa: F401,F403
from .frame import *  # noqa: F401,F403
from .crf import *  # noqa: F401,F403
from .knn import *  # noqa: F401,F403
from .segloss import *  # noqa: F401,F403
from .fire import *  # noqa: F401,F403
from .cam import *  # noqa: F401,F403
from .sgd import *  # noqa: F401,F403
from .render import *  # noqa: F401,F403
from .latent import *  # noqa: F401,F403
from .syncbn import *  # noqa: F401,F403
from .pointnet import *  # noqa: F401,F403
from .upsample import *  # noqa: F401,F403
