"""RAG-side components (hilbert_quantization.rag.*) backed by libhq_mi355x.

QuantizedFrameCorpus searches the store's u8 frames in place with u8 queries (search, search_parameters) and with
float32 queries at full precision (search_float, search_parameters(quantize_query=False)).
ComprehensiveFrameCorpus ranks enhanced frames by the engine's comprehensive similarity (hierarchical + embedding +
spatial), fused into one matrix-core contraction for a store written by one generator.
HierarchicalFrameCorpus runs the engine's progressive hierarchical search (the candidate cascade over the index rows
that precedes that ranking) for whole query batches on the device."""
from .hilbert_mapper import HilbertCurveMapperImpl
from .hierarchical_index_generator import HierarchicalIndexGenerator
from .similarity import (ComprehensiveFrameCorpus, FrameCosineCorpus, HierarchicalFrameCorpus, QuantizedFrameCorpus,
                         apply_progressive_threshold, progressive_hierarchical_search,
                         calculate_comprehensive_similarity, calculate_embedding_similarity, comprehensive_scores,
                         comprehensive_scores_listed,
                         similarity_weights,
                         calculate_embedding_cosine_similarity, calculate_granularity_weights, calculate_spatial_locality_similarity,
                         compare_multi_level_indices, compare_single_level_indices, cosine_scores_batch,
                         cosine_topk_batch, detect_original_embedding_height, extract_original_embedding,
                         progressive_threshold, progressive_threshold_batch, spatial_locality_scores)

__all__ = ["ComprehensiveFrameCorpus", "HierarchicalFrameCorpus", "progressive_hierarchical_search", "calculate_comprehensive_similarity", "calculate_embedding_similarity",
           "comprehensive_scores", "comprehensive_scores_listed", "similarity_weights", "FrameCosineCorpus", "HilbertCurveMapperImpl", "HierarchicalIndexGenerator", "QuantizedFrameCorpus",
           "apply_progressive_threshold",
           "calculate_embedding_cosine_similarity", "calculate_granularity_weights",
           "calculate_spatial_locality_similarity", "compare_multi_level_indices", "compare_single_level_indices",
           "cosine_scores_batch", "cosine_topk_batch", "detect_original_embedding_height",
           "extract_original_embedding",
           "progressive_threshold", "progressive_threshold_batch", "spatial_locality_scores"]
