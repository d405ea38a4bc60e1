"""Reference-shaped core components (hilbert_quantization.core.*) backed by libhq_mi355x."""
from .dimension_calculator import PowerOf4DimensionCalculator
from .hilbert_mapper import HilbertCurveMapper
from .streaming_index_builder import StreamingHilbertIndexGenerator
from .index_generator import HierarchicalIndexGeneratorImpl
from .compressor import MPEGAICompressorImpl
from .search_engine import ProgressiveSimilaritySearchEngine, LevelConfig, IndexCorpus
from .pipeline import QuantizationPipeline, quantize_batch
from .precomputed_hilbert_index import (PrecomputedHilbertIndexer, PrecomputedSimilaritySearchEngine,
                                        PrecomputedIndex, PrecomputedLevel)
from .frame_order import (FrameOrdering, sort_frames_by_hierarchical_indices, frame_ordering_metrics,
                          find_optimal_insertion_position)
from .cv_features import calculate_ssim, ssim_scores, ssim_scores_listed, template_correlation
from .video_search import VideoFeatureIndex, extract_video_features

__all__ = ["PowerOf4DimensionCalculator", "HilbertCurveMapper", "StreamingHilbertIndexGenerator",
           "HierarchicalIndexGeneratorImpl", "MPEGAICompressorImpl", "ProgressiveSimilaritySearchEngine",
           "LevelConfig", "IndexCorpus", "QuantizationPipeline", "quantize_batch", "PrecomputedHilbertIndexer",
           "PrecomputedSimilaritySearchEngine", "PrecomputedIndex", "PrecomputedLevel", "FrameOrdering",
           "sort_frames_by_hierarchical_indices", "frame_ordering_metrics", "find_optimal_insertion_position",
           "calculate_ssim", "ssim_scores", "ssim_scores_listed", "template_correlation",
           "VideoFeatureIndex", "extract_video_features"]
