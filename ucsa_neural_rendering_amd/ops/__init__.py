"""Tensor-level wrappers over the C ABI (``include/ucsa_hip.h``).

PyTorch is used for device memory and streams only: every function checks its
arguments, allocates outputs with ``torch.empty`` and enqueues the HIP kernels
on torch's current stream.  No arithmetic happens here.

The wrappers live in one module per family (``render``, ``backward``, ``train``,
``march``, ``volume``, ``mesh``, ``search``) over the shared argument checks of
``_args``; this file only re-exports them, so ``ops.NAME`` is the way in.
``raycast`` came after the surface of ``ops`` was frozen and is reached as a
module: ``ops.raycast.raycast_mesh``; so is ``register``: ``ops.register.icp_sums``,
``ops.register.tsdf_sums``, ``ops.register.projective_sums``, ``ops.register.tsdf_scores``; and ``depth``:
``ops.depth.depth_frontend``, ``ops.depth.pyramid_down``.
"""
from .. import _lib
from .._lib import Grid, check, fvec, lib
from . import _args, backward, depth, march, mesh, raycast, register, render, search, train, volume
from ._args import (_march_ws, _named_ws, _ptr, _scratch, _scratch_named, _stream,
                    volume_lattice)
from .backward import *          # noqa: F401,F403  (the modules define no __all__:
from .backward import _bwd_ws    # noqa: F401        every public name is an op)
from .march import *             # noqa: F401,F403
from .mesh import *              # noqa: F401,F403
from .render import *            # noqa: F401,F403
from .search import *            # noqa: F401,F403
from .train import *             # noqa: F401,F403
from .volume import *            # noqa: F401,F403
