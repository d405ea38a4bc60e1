"""The drop-in joins the reference's type hierarchy when the reference package is importable (SURVEY §7
step 3, VERDICT r02 missing item 7): exceptions subclass the reference's, components subclass its ABCs
(interfaces.py:12-225) and the data model is its own dataclasses (models.py:11-80).  Checked in child
processes: with a minimal stand-in package named hilbert_quantization (the reference's class and field
names, none of its code), and without any (own types)."""
import os
import subprocess
import sys
import textwrap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hilbert-quantization_amd")

CHECK = textwrap.dedent("""
    import sys, numpy as np
    sys.path.insert(0, %r)
    import hilbert_quantization.exceptions as RE, hilbert_quantization.interfaces as RI, hilbert_quantization.models as RM
    from hq_mi355x import exceptions as E, models as M
    from hq_mi355x.core.hilbert_mapper import HilbertCurveMapper
    from hq_mi355x.core.index_generator import HierarchicalIndexGeneratorImpl
    from hq_mi355x.core.compressor import MPEGAICompressorImpl
    from hq_mi355x.core.search_engine import ProgressiveSimilaritySearchEngine
    from hq_mi355x.core.dimension_calculator import PowerOf4DimensionCalculator
    for n in ("HilbertQuantizationError", "QuantizationError", "SearchError", "ReconstructionError", "ValidationError",
              "CompressionError"):
        assert issubclass(getattr(E, n), getattr(RE, n)), n
        assert issubclass(getattr(E, n), E.HilbertQuantizationError), n
    try:
        raise E.QuantizationError("x")
    except RE.QuantizationError:
        pass
    assert isinstance(HilbertCurveMapper(), RI.HilbertCurveMapper)
    assert isinstance(HierarchicalIndexGeneratorImpl(), RI.HierarchicalIndexGenerator)
    assert isinstance(MPEGAICompressorImpl(), RI.MPEGAICompressor)
    assert isinstance(ProgressiveSimilaritySearchEngine(), RI.SimilaritySearchEngine)
    assert isinstance(PowerOf4DimensionCalculator(), RI.DimensionCalculator)
    assert M.QuantizedModel is RM.QuantizedModel and M.SearchResult is RM.SearchResult
    md = M.ModelMetadata("m", 1, 1, 1.0, "t")
    qm = M.QuantizedModel(b"x", (8, 8), 4, 0.8, np.zeros(8), md)
    assert qm.model_id == "m"
    print("bound")
""") % PKG


def _run(code, extra_path=None, env=None):
    e = dict(os.environ)
    e.pop("HQ_NO_REFERENCE_BINDING", None)
    e["PYTHONPATH"] = os.pathsep.join(p for p in (extra_path, e.get("PYTHONPATH")) if p)
    e["PYTHONDONTWRITEBYTECODE"] = "1"
    if env:
        e.update(env)
    return subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=e, timeout=300)


STAND_IN = {
    "__init__.py": "",
    "exceptions.py": "\n".join(f"class {n}({b}):\n    pass\n" for n, b in (
        ("HilbertQuantizationError", "Exception"), ("DimensionCalculationError", "HilbertQuantizationError"),
        ("HilbertMappingError", "HilbertQuantizationError"), ("IndexGenerationError", "HilbertQuantizationError"),
        ("CompressionError", "HilbertQuantizationError"), ("SearchError", "HilbertQuantizationError"),
        ("ValidationError", "HilbertQuantizationError"), ("ConfigurationError", "HilbertQuantizationError"),
        ("QuantizationError", "HilbertQuantizationError"), ("ReconstructionError", "HilbertQuantizationError"))),
    "interfaces.py": textwrap.dedent("""
        from abc import ABC, abstractmethod
        class DimensionCalculator(ABC):
            @abstractmethod
            def calculate_optimal_dimensions(self, param_count): ...
            @abstractmethod
            def calculate_padding_strategy(self, param_count, target_dims): ...
        class HilbertCurveMapper(ABC):
            @abstractmethod
            def map_to_2d(self, parameters, dimensions): ...
            @abstractmethod
            def map_from_2d(self, image): ...
            @abstractmethod
            def generate_hilbert_coordinates(self, n): ...
        class HierarchicalIndexGenerator(ABC):
            @abstractmethod
            def generate_optimized_indices(self, image, index_space_size): ...
            @abstractmethod
            def calculate_level_allocation(self, total_space): ...
            @abstractmethod
            def calculate_spatial_averages(self, image, grid_size): ...
            @abstractmethod
            def embed_indices_in_image(self, image, indices): ...
        class MPEGAICompressor(ABC):
            @abstractmethod
            def compress(self, image, quality): ...
            @abstractmethod
            def decompress(self, compressed_data): ...
            @abstractmethod
            def estimate_compression_ratio(self, original_size, compressed_size): ...
        class SimilaritySearchEngine(ABC):
            @abstractmethod
            def progressive_search(self, query_indices, candidate_pool, max_results): ...
            @abstractmethod
            def compare_indices_at_level(self, query_indices, candidate_indices, level): ...
    """),
    "models.py": textwrap.dedent("""
        from dataclasses import dataclass
        from typing import Any, Optional
        import numpy as np
        @dataclass
        class ModelMetadata:
            model_name: str
            original_size_bytes: int
            compressed_size_bytes: int
            compression_ratio: float
            quantization_timestamp: str
            model_architecture: Optional[str] = None
            additional_info: Optional[dict] = None
            compression_metrics: Optional[Any] = None
        @dataclass
        class PaddingConfig:
            target_dimensions: tuple
            padding_value: float
            padding_positions: list
            efficiency_ratio: float
        @dataclass
        class QuantizedModel:
            compressed_data: bytes
            original_dimensions: tuple
            parameter_count: int
            compression_quality: float
            hierarchical_indices: np.ndarray
            metadata: ModelMetadata
            @property
            def model_id(self):
                return self.metadata.model_name
        @dataclass
        class SearchResult:
            model: QuantizedModel
            similarity_score: float
            matching_indices: dict
            reconstruction_error: float
    """),
}


def test_binds_to_stand_in_reference(tmp_path):
    pkg = tmp_path / "hilbert_quantization"
    pkg.mkdir()
    for name, text in STAND_IN.items():
        (pkg / name).write_text(text)
    r = _run(CHECK, str(tmp_path))
    assert r.returncode == 0 and "bound" in r.stdout, r.stderr[-3000:]


def test_own_types_without_reference():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from hq_mi355x import exceptions as E, models as M, _compat\n"
            "assert _compat.reference_module('models') is None\n"
            "assert E.QuantizationError.__mro__[1] is E.HilbertQuantizationError\n"
            "assert M.QuantizedModel.__module__ == 'hq_mi355x.models'\n"
            "print('own')\n") % PKG
    r = _run(code, env={"HQ_NO_REFERENCE_BINDING": "1"})
    assert r.returncode == 0 and "own" in r.stdout, r.stderr[-3000:]
