from .icp_optimzier import ICP_Optimizer  # noqa: F401
from .lap_deform_optimizer import Laplacian_Optimizer  # noqa: F401
from .nricp_optimizer import Local_Affine, NRICP_Optimizer_AdamW, TriMesh  # noqa: F401
from .surface_intesection import Surface_Intesection  # noqa: F401
