"""rovinasemanticsegmentation_amd -- MI355X-native per-pixel RF + DenseCRF inference path.

Host-side mirror of the reference's Segmenter hot loop over librvseg.so (HIP, gfx950).
`import torch` before this package if the process also uses torch, so that both share one HIP
runtime.  There is no CPU fallback: without the built library the import of `_capi.lib()` fails,
without a GPU `Context()` raises.
"""
from . import _capi as capi  # noqa: F401
from ._capi import projection_matrix  # noqa: F401
from .segmenter import (BoostedRandomForest, Context, DenseCRF, Evaluator, FeatureExtractor, LocalMapStore, RandomForest,  # noqa: F401
                        RgbLabelConversion, Segmenter, PottsCompatibility, DiagonalCompatibility, MatrixCompatibility,
                        CONST_KERNEL, DIAG_KERNEL, FULL_KERNEL, NO_NORMALIZATION, NORMALIZE_BEFORE, NORMALIZE_AFTER,
                        NORMALIZE_SYMMETRIC, LogLikelihood, Hamming, IntersectionOverUnion, CRFEnergy, CRFKernelEnergy,
                        minimizeLBFGS, numericGradient, gradCheck, AccuracyTool, ConfusionMatrixTool, CorrelationTool, RandomForestPrune)
from . import synthetic  # noqa: F401

__all__ = ["capi", "BoostedRandomForest", "Context", "DenseCRF", "FeatureExtractor", "LocalMapStore", "RandomForest", "Segmenter", "synthetic",
           "RgbLabelConversion", "Evaluator", "PottsCompatibility", "DiagonalCompatibility", "MatrixCompatibility",
           "CONST_KERNEL", "DIAG_KERNEL", "FULL_KERNEL", "NO_NORMALIZATION", "NORMALIZE_BEFORE", "NORMALIZE_AFTER",
           "NORMALIZE_SYMMETRIC", "projection_matrix", "LogLikelihood", "Hamming", "IntersectionOverUnion",
           "CRFEnergy", "CRFKernelEnergy", "minimizeLBFGS", "numericGradient", "gradCheck", "AccuracyTool", "ConfusionMatrixTool",
           "CorrelationTool", "RandomForestPrune"]
