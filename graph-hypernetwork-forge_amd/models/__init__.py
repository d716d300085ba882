"""Host mirrors of the reference's modules (same constructors, attributes, state_dict keys and call signatures); every
forward and backward runs in libghf_hip.so."""

from .hypergnn import GraphedForward, HyperGNN, TextEncoder, link_prediction_metrics
from .relation_decoder import RelationDecoder
from .weight_generator import WeightGenerator

__all__ = ("HyperGNN", "WeightGenerator", "TextEncoder", "GraphedForward", "link_prediction_metrics", "RelationDecoder")
