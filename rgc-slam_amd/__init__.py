"""rgc-slam_amd -- MI355X-native scan-to-map registration path for RGC-SLAM.

Holds only what the hot path needs: ``csrc/`` (HIP kernels + C-ABI ``librgc_hip.so``), the
host-side mirror of the reference's registration interface (``registration.FastVGICP``), the
ctypes binding (``_lib``), the search index (``search.KdTree``: exact k-NN and radius search of arbitrary queries), the outlier filters
(``filters.StatisticalOutlierRemoval`` / ``filters.RadiusOutlierRemoval``), Euclidean cluster extraction and RANSAC plane segmentation
(``segmentation.EuclideanClusterExtraction`` / ``segmentation.SACSegmentation``), surface normal estimation and FPFH descriptors (``features.NormalEstimation`` / ``features.FPFHEstimation``)
and the synthetic data generator (``synth``; data only).
"""
__all__ = ["synth", "search", "filters", "segmentation", "features"]
