from .activations import shifted_softplus
from .base import Dense
from .blocks import Residual, ResidualMLP, ResidualStack, build_gated_equivariant_mlp, build_mlp
from .embedding import ElectronicEmbedding, NuclearEmbedding
from .equivariant import GatedEquivariantBlock
from .cutoff import CosineCutoff, SwitchFunction, cosine_cutoff
from .radial import BesselRBF, GaussianRBF, gaussian_rbf
from .scatter import scatter_add
from .so3 import (RealSphericalHarmonics, SO3Convolution, SO3GatedNonlinearity, SO3ParametricGatedNonlinearity, SO3TensorProduct, scalar2rsh,
                  sh_indices)
from .utils import replicate_module
