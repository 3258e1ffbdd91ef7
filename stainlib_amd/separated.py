"""Separated: what the stain separation returns (engine.stain_separate, the normalizers' separate / separate_batch)."""
import collections

Separated = collections.namedtuple("Separated", ("norm", "h", "e", "conc"), defaults=(None, None, None, None))
Separated.__doc__ = """The normalised image, the haematoxylin-only and the eosin-only image ((N,H,W,3) uint8 each) and the concentration
planes ((N,2,H,W), haematoxylin first); None for what was not wanted."""
