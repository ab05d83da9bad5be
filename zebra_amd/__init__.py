"""zebra_amd -- MI355X (gfx950) implementation of Zebra's hot path:
streaming / pruning top-k T-PPR, top-k gather + aggregate, TGN memory update.

The compute lives in zebra_amd/lib/libzebra_amd.so (hand-written HIP, C-ABI in
include/zebra_amd.h).  The Python classes mirror the reference's surface.
"""
__version__ = "0.1.0"


def __getattr__(name):
    # (resolved on first use: `python -m zebra_amd.build` imports the package and needs no torch)
    if name == "Adam":
        from .optim import Adam
        return Adam
    if name == "link_bce_loss":
        from .losses import link_bce_loss
        return link_bce_loss
    if name == "label_bce_loss":
        from .losses import label_bce_loss
        return label_bce_loss
    if name == "listwise_loss":
        from .losses import listwise_loss
        return listwise_loss
    if name == "MLP":
        from .decoder import MLP
        return MLP
    if name == "NegativeSampler":
        from .sampling import NegativeSampler
        return NegativeSampler
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
