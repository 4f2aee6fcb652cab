"""mio -- MI355X-native transformer-inference hot path (FA3 attention, FusedMLP, ring attention,
tensor-parallel all-reduce) behind the reference's operator surface.

Importing the kernel-backed modules loads libmio_hip.so through ctypes (mio._lib); there is no
CPU / PyTorch fallback for the compute path.
"""
__version__ = "0.1.0"


def __getattr__(name):
    # Sampler lives in mio.sampling, which loads the library: resolved on first use so that `import mio` stays light
    if name == "Sampler":
        from .sampling import Sampler
        return Sampler
    raise AttributeError(f"module 'mio' has no attribute {name!r}")
