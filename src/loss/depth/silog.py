from dualpixelface_amd.losses import SILOGLoss  # noqa: F401
