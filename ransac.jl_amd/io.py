"""Wire formats either side of the hot path, compatible with the reference's
(src/json-yaml.jl): `toDict` / `exportJSON` for shapes and `readconfig` for YAML configs."""
import json

import numpy as np

from .api import (DEFAULT_PARAMETERS, DEFAULT_SHAPE_DICT, ExtractedShape, FittedCone, FittedCylinder, FittedPlane,
                  FittedShape, FittedSphere, ransacparameters, strt)

# field order = fieldnames(typeof(s)) of the reference structs (shapes/*.jl)
_FIELDS = {FittedPlane: ("point", "normal"), FittedSphere: ("center", "radius", "outwards"),
           FittedCylinder: ("axis", "center", "radius", "outwards"), FittedCone: ("apex", "axis", "opang", "outwards")}


def _extent_dict(e):
    return {"origin": [float(x) for x in e.origin], "frame": [[float(x) for x in row] for row in e.frame],
            "lo": [float(x) for x in e.lo], "hi": [float(x) for x in e.hi], "centroid": [float(x) for x in e.centroid],
            "rms": float(e.dist_rms), "maxabs": float(e.dist_maxabs)}


def toDict(s, extents=False):
    """toDict(s) (json-yaml.jl:9-30): {"type": strt(s), <field>: value ...}; a list of shapes /
    ExtractedShapes becomes {"primitives": [...]}.  extents=True: an ExtractedShape that carries an `.extent`
    (ransac(..., extents=True), shape_extents) also gets an "extent" entry -- origin, frame (rows u, v, w), lo, hi,
    centroid, rms, maxabs; without it the output is the reference's."""
    if isinstance(s, (list, tuple)):
        return {"primitives": [toDict(x, extents) for x in s]}
    if isinstance(s, ExtractedShape):
        d = toDict(s.shape)
        if extents and getattr(s, "extent", None) is not None:
            d["extent"] = _extent_dict(s.extent)
        return d
    if not isinstance(s, FittedShape):
        raise TypeError("toDict expects a FittedShape, an ExtractedShape or a list of them")
    d = {"type": strt(s)}
    for f in _FIELDS[type(s)]:
        v = getattr(s, f)
        d[f] = [float(x) for x in v] if isinstance(v, np.ndarray) else v
    return d


def exportJSON(io, s, indent=None, extents=False):
    """exportJSON(io, s[, indent]) (json-yaml.jl:43-59); extents: see toDict."""
    if indent is None:
        io.write(json.dumps(toDict(s, extents), separators=(",", ":")))
    else:
        io.write(json.dumps(toDict(s, extents), indent=indent) + "\n")


def _dict2nt(v):
    """dict2nt (json-yaml.jl:98-109): a YAML list of single-key maps merged into one dict."""
    out = {}
    for d in v:
        out.update(d)
    return out


def readconfig(fname, toextend=None, shapedict=None):
    """readconfig(fname; toextend=DEFAULT_PARAMETERS, shapedict=DEFAULT_SHAPE_DICT) (json-yaml.jl:81-96)."""
    import yaml
    toextend = DEFAULT_PARAMETERS if toextend is None else toextend
    shapedict = DEFAULT_SHAPE_DICT if shapedict is None else shapedict
    with open(fname, "r", encoding="utf-8") as f:
        fdict = yaml.safe_load(f)
    for k, v in fdict.items():
        nt = _dict2nt(v)
        if "shape_types" in nt:
            nt = dict(nt)
            nt["shape_types"] = [shapedict[name] for name in nt["shape_types"]]
        toextend = ransacparameters(toextend, **{k: nt})
    return toextend
