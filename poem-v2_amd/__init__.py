"""MI355X-native point-embedded decoder for POEM-v2 (hot path only).

Public surface mirrors the reference's plugin API for this path: ``HEAD`` / ``TRANSFORMER`` registries,
``build_head`` / ``build_transformer``, classes ``POEM_Generalized_Head`` and ``PtEmbedTRv4`` (importing the package
registers them, as ``import lib.models`` does upstream)."""
from .config import CN  # noqa: F401
from .builder import (HEAD, TRANSFORMER, BACKBONE, MODEL, Registry, build_from_cfg, build_head, build_transformer,  # noqa: F401
                      build_backbone, build_model)
from . import builder, weights, inputs, hip, configs, triangulation, decode, backbone, resnet, jpeg, transform, wds, mano, render, losses  # noqa: F401
from .transformer import PtEmbedTRv4  # noqa: F401
from .head import POEM_Generalized_Head  # noqa: F401
from .backbone import HRNet  # noqa: F401
from .resnet import ResNet18, ResNet34, ResNet50  # noqa: F401
from .model import PtEmbedMultiviewStereoV2  # noqa: F401
from .transform import TRANSFORM, SimpleTransform3DMultiView, build_transform  # noqa: F401
from .wds import MultiviewWebDataset, MixWebDataset, collation_random_n_views  # noqa: F401
from .jpeg import EncodedImage  # noqa: F401
from .mano import ManoLayer  # noqa: F401
from . import fit  # noqa: F401
from .fit import ManoFit, fit_mano  # noqa: F401
from .hip import make_basis  # noqa: F401
from .render import MeshRenderer, DrawingHandCallback, draw_skeleton, project_to_views, save_png  # noqa: F401
from .losses import PoemLoss, LossMetric  # noqa: F401
from . import metrics  # noqa: F401
from .metrics import MeshFScore, PAJoint3DPCK, PAVert3DPCK, procrustes_align, nearest_distances  # noqa: F401
