"""rl4co_amd — MI355X-native autoregressive rollout engine for the RL4CO hot path.

The package mirrors the reference's Python surfaces for that path only
(``RL4COEnvBase.reset/step/get_reward`` and ``AutoregressivePolicy.forward``) on top of
hand-written HIP kernels for gfx950 reached through a C-ABI (``include/rl4co_amd.h``).
See DESIGN.md for the path, the boundary and what is out of scope.
"""
__version__ = "0.1.0"

__all__ = ["AntSystem", "DeepACOPolicy", "GFACSDepotEncoder", "GFACSEncoder", "GFACSPolicy", "NARGNNDepotEncoder",
           "NARGNNEncoder", "NARGNNPolicy", "NonAutoregressivePolicy", "TrainableNARGNNDepotEncoder", "TrainableNARGNNEncoder", "gfacs_alpha",
           "gfacs_beta", "gfacs_loss", "log_pb_uniform"]


def __getattr__(name):
    if name == "AntSystem":  # rl4co_amd.aco: the reference's AntSystem on the rl4co_aco_tsp kernel (imported on first use)
        from .aco import AntSystem

        return AntSystem
    if name in ("gfacs_loss", "log_pb_uniform", "gfacs_alpha", "gfacs_beta"):  # rl4co_amd.aco: GFACS's trajectory-balance loss
        from . import aco

        return getattr(aco, name)
    # rl4co_amd.nargnn: DeepACO's heatmap encoders on rl4co_nargnn_heatmap / rl4co_nargnn_depot_heatmap
    if name in ("NARGNNEncoder", "NARGNNDepotEncoder", "DeepACOPolicy", "NonAutoregressivePolicy", "TrainableNARGNNEncoder",
                "TrainableNARGNNDepotEncoder", "GFACSEncoder", "GFACSDepotEncoder", "GFACSPolicy", "NARGNNPolicy"):
        from . import nargnn

        return getattr(nargnn, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
