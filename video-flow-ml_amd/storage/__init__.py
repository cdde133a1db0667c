"""storage — flow cache files and naming (mirror of the reference's storage/ package)."""
from .cache_manager import FlowCacheManager, FlowFileHandler, LODGenerator
from .async_writer import AsyncFlowCacheWriter
from .avi_writer import AviWriter
from .avi_reader import AviReader

__all__ = ["FlowCacheManager", "FlowFileHandler", "LODGenerator", "AsyncFlowCacheWriter", "AviWriter", "AviReader"]
