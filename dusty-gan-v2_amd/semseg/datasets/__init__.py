from .sqsg import GTALiDAR, GTALiDAR_GAN, KITTIRawFrontal, SyntheticFrontal  # noqa: F401

__all__ = ["GTALiDAR", "GTALiDAR_GAN", "KITTIRawFrontal", "SyntheticFrontal"]
