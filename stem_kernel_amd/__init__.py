"""MI355X-native stem-kernel Gram engine (gfx950 HIP kernels behind a C ABI).

See include/stem_kernel.h for the ABI and DESIGN.md for the design.
"""
from ._lib import StemKernelError, lib, default_params  # noqa: F401
from .kernel_matrix import (  # noqa: F401
    BPLAKernel, Context, Dataset, KernelMatrix, LAKernel, SVMModel, LSuStemKernel, LSuStemStrKernel, NaiveStringKernel, SiStemKernel,
    SiStemStrKernel, SimpalKernel, StemKernel4D, StemStrKernel, StringKernel, SuStemKernel, SuStemStrKernel, fold,
    format_libsvm, parse_examples, random_sequences, read_examples, simpal_shape,
)
from .svm import (  # noqa: F401
    DEFAULT_MAX_ITER, AUCGradient, CrossValidation, SVMSolution, auc_delta, auc_gradient_batch,
    auc_gradient_shape, auc_objective, cross_validate, cv_split, optimize, svm_train, svm_train_batch,
    svm_solve_shape, svm_train_shape,
)

from .features import (  # noqa: F401
    FeatureSet, PolyKernel, RBFKernel, SigmoidKernel, feature_auc_objective, feature_dots, feature_gram,
    feature_gram_cross, feature_gram_shape, optimize_features,
)
from .la_grad import (  # noqa: F401
    la_auc_objective, la_grad_shape, la_gradient_gram, la_gradients, optimize_la,
)
from .stem_grad import (  # noqa: F401
    optimize_stem, stem_auc_objective, stem_gradient_gram, stem_gradients,
)

__version__ = "0.1.0"
