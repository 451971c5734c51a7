from .nricp_optimizer import Local_Affine, NRICP_Optimizer_AdamW, TriMesh  # noqa: F401
