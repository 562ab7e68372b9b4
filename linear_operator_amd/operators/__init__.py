"""The operator classes that feed the iterative solve / logdet path."""
from ._linear_operator import LinearOperator, to_dense
from .added_diag_linear_operator import AddedDiagLinearOperator
from .constant_mul_linear_operator import ConstantMulLinearOperator
from .dense_linear_operator import DenseLinearOperator, to_linear_operator
from .diag_linear_operator import ConstantDiagLinearOperator, DiagLinearOperator
from .identity_linear_operator import IdentityLinearOperator
from .interpolated_linear_operator import InterpolatedLinearOperator
from .kronecker_product_linear_operator import KroneckerProductDiagLinearOperator, KroneckerProductLinearOperator
from .kronecker_product_added_diag_linear_operator import KroneckerProductAddedDiagLinearOperator
from .linear_operator_representation_tree import LinearOperatorRepresentationTree
from .low_rank_root_added_diag_linear_operator import LowRankRootAddedDiagLinearOperator
from .matmul_linear_operator import MatmulLinearOperator
from .mul_linear_operator import MulLinearOperator
from .root_linear_operator import LowRankRootLinearOperator, RootLinearOperator
from .sum_linear_operator import PsdSumLinearOperator, SumLinearOperator
from .sum_kronecker_linear_operator import SumKroneckerLinearOperator
from .toeplitz_linear_operator import ToeplitzLinearOperator
from .triangular_linear_operator import TriangularLinearOperator
from .chol_linear_operator import CholLinearOperator
from .block_linear_operator import BlockLinearOperator
from .block_diag_linear_operator import BlockDiagLinearOperator
from .block_interleaved_linear_operator import BlockInterleavedLinearOperator
from .sum_batch_linear_operator import SumBatchLinearOperator
from .masked_linear_operator import MaskedLinearOperator
from .kernel_linear_operator import KernelLinearOperator

__all__ = [
    "LowRankRootAddedDiagLinearOperator", "KroneckerProductAddedDiagLinearOperator",
    "LinearOperator", "to_dense", "to_linear_operator", "AddedDiagLinearOperator", "DenseLinearOperator",
    "DiagLinearOperator", "ConstantDiagLinearOperator", "IdentityLinearOperator", "KroneckerProductLinearOperator", "KroneckerProductDiagLinearOperator",
    "LinearOperatorRepresentationTree", "RootLinearOperator", "LowRankRootLinearOperator", "SumLinearOperator",
    "PsdSumLinearOperator", "TriangularLinearOperator", "MatmulLinearOperator", "InterpolatedLinearOperator",
    "ToeplitzLinearOperator", "ConstantMulLinearOperator", "MulLinearOperator", "CholLinearOperator",
    "BlockLinearOperator", "BlockDiagLinearOperator", "BlockInterleavedLinearOperator", "SumBatchLinearOperator",
    "MaskedLinearOperator", "SumKroneckerLinearOperator", "KernelLinearOperator",
]
