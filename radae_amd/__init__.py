"""radae_amd -- MI355X-native implementation of the RADAE streaming hot path.

Only what the path needs: csrc/ (HIP kernels + C ABI), abi.py (the C ABI as ctypes, stated once),
engine.py and stages.py (binding of the batched C ABI: the engine proper, the front-end stages), api.py (mirror of the reference's radae_tx / radae_rx Python classes over rade_api.h),
dnnw.py (weight-blob reader), channel_tools.py (Doppler/feature generators), loss.py.
"""
__all__ = ["engine", "api", "dnnw", "channel_tools", "loss"]
