"""Reads the reference's parameter files UNCHANGED into a te_params block (+ the run flags the chain's tail implies).

What the ROS node does with these files (reference, file:line):
  * `robot_filter_parameter.yaml` -- the list `traversability_map_filters` is what `filters::FilterChain::configure`
    walks (`TE/src/TraversabilityMap.cpp:129-131`); each entry's `params` are read by the plugin's `configure()`
    (`TEF/src/SlopeFilter.cpp:34-56`, `StepFilter.cpp:38-99`, `RoughnessFilter.cpp:36-70`).
  * `robot_footprint_parameter.yaml` -- `footprint/...` (`TE/src/TraversabilityMap.cpp:92-126`).
  * `robot.yaml` -- `max_gap_width` (`TraversabilityMap.cpp:117`).

The chain this library runs is the fixed sequence normals -> slope -> step -> roughness -> weighted sum -> deletion; a file
that asks for anything else (another order, another filter type, an expression that is not a weighted sum of the three
scores, an input layer other than `elevation`) is refused with a message rather than half-applied.  An expression of any other
form is served by `params_and_expression_from_yaml`: the chain runs with default weights and the text goes to
`Context.run_expression` (te_run_expression) behind it.  Host-side plumbing
for bench.py and the tests: the plugins themselves get their parameters from `FilterBase::getParam`, as in the reference.
"""
import re

import numpy as np

CHAIN_KEY = "traversability_map_filters"
_NUM = r"[-+]?(?:\d+\.?\d*(?:[eE][-+]?\d+)?|\.\d+(?:[eE][-+]?\d+)?)"
_SCORES = {"traversability_slope": "w_slope", "traversability_step": "w_step", "traversability_roughness": "w_rough"}


class ParamsYamlError(ValueError):
    pass


def _load(path_or_text):
    import yaml
    if "\n" not in str(path_or_text):
        with open(path_or_text) as f:
            return yaml.safe_load(f)
    return yaml.safe_load(path_or_text)


def _scalar_f32(text):
    """`1.0 / 3.0`, `0.25`, `(1.0/3.0)`: evaluated in float32 like EigenLab does on MatrixXf scalars."""
    t = text.strip()
    while t.startswith("(") and t.endswith(")"):
        t = t[1:-1].strip()
    m = re.fullmatch(rf"({_NUM})\s*/\s*({_NUM})", t)
    if m:
        return np.float32(np.float32(float(m.group(1))) / np.float32(float(m.group(2))))
    if re.fullmatch(_NUM, t):
        return np.float32(float(t))
    raise ParamsYamlError(f"weighted sum: cannot read the scalar '{text}'")


def parse_weighted_sum(expression, names=_SCORES):
    """`scale * (a + b + c)` with optional per-layer factors `w * layer`; returns {"w_scale", "w_slope", "w_step", "w_rough"}
    as float32.  The shipped expression (`robot_filter_parameter.yaml:33`) gives (1.0f/3.0f, 1, 1, 1)."""
    e = expression.strip()
    m = re.fullmatch(r"(.+?)\*\s*\((.+)\)", e)
    scale, body = (np.float32(1.0), e) if not m else (_scalar_f32(m.group(1)), m.group(2))
    if not m and e.startswith("(") and e.endswith(")"):
        body = e[1:-1]
    out = {"w_scale": scale}
    order = []
    for term in body.split("+"):
        t = term.strip()
        mm = re.fullmatch(rf"(?:(.+?)\*\s*)?([A-Za-z_][A-Za-z_0-9]*)", t)
        if not mm or mm.group(2) not in names:
            raise ParamsYamlError(f"weighted sum: '{t}' is not a (weighted) score layer of the chain")
        key = names[mm.group(2)]
        if key in out:
            raise ParamsYamlError(f"weighted sum: layer '{mm.group(2)}' appears twice")
        out[key] = np.float32(1.0) if mm.group(1) is None else _scalar_f32(mm.group(1))
        order.append(key)
    if order != ["w_slope", "w_step", "w_rough"]:
        # float32 addition is not associative: the kernel evaluates ((slope + step) + roughness), left to right like EigenLab
        raise ParamsYamlError("weighted sum: the three score layers must appear once each, in the order slope + step + roughness")
    return out


def _axis(v):
    try:
        return {"x": 0, "y": 1, "z": 2}[str(v).strip().lower()]
    except KeyError:
        raise ParamsYamlError(f"normal_vector_positive_axis must be x, y or z (got '{v}')")


def filter_chain_fields(doc, general_expression=False):
    """te_params fields (plain dict) + {"keep_normals": bool, "normals_algorithm": 0 | 1} from the `traversability_map_filters`
    list.  normals_algorithm is NormalVectorsFilter's `algorithm` key (area: 0, the default; raster: 1), the value of
    TE_OPT_NORMALS_ALGORITHM: an option of the context, no field of te_params.
    general_expression: an expression parse_weighted_sum refuses leaves the four weights out (their defaults hold) instead
    of raising: the caller hands the text to te_run_expression."""
    if not isinstance(doc, dict) or CHAIN_KEY not in doc:
        raise ParamsYamlError(f"no '{CHAIN_KEY}' list in the filter parameter file")
    chain = doc[CHAIN_KEY]
    want = ["gridMapFilters/NormalVectorsFilter", "traversabilityFilters/SlopeFilter", "traversabilityFilters/StepFilter",
            "traversabilityFilters/RoughnessFilter", "gridMapFilters/MathExpressionFilter"]
    types = [str(f.get("type")) for f in chain]
    if types[:5] != want or types[5:] not in ([], ["gridMapFilters/DeletionFilter"]):
        raise ParamsYamlError("the filter chain must be NormalVectorsFilter, SlopeFilter, StepFilter, RoughnessFilter, MathExpressionFilter"
                              f" [, DeletionFilter] in this order (got {types})")
    prm = [f.get("params") or {} for f in chain]
    nrm, slope, step, rough, comb = prm[:5]

    def need(d, key, who):
        if key not in d:
            raise ParamsYamlError(f"{who} did not find param {key}")  # the reference's ROS_ERROR wording
        return d[key]

    if str(nrm.get("input_layer", "elevation")) != "elevation":
        raise ParamsYamlError("NormalVectorsFilter: input_layer must be 'elevation'")
    prefix = str(nrm.get("output_layers_prefix", "surface_normal_"))
    if prefix != "surface_normal_":
        raise ParamsYamlError("NormalVectorsFilter: output_layers_prefix must be 'surface_normal_' (SlopeFilter.cpp:71 hard-codes it)")
    try:
        algorithm = {"area": 0, "raster": 1}[str(nrm.get("algorithm", "area"))]
    except KeyError:
        raise ParamsYamlError(f"NormalVectorsFilter: algorithm must be area or raster (got '{nrm.get('algorithm')}')")
    out = {}
    # (upstream reads `radius` for the area method only: a raster file may leave it out, and te_params_default's value stays)
    if algorithm == 0 or "radius" in nrm:
        out["normals_radius"] = float(need(nrm, "radius", "Normal vectors filter"))
    out.update({"normals_axis": _axis(nrm.get("normal_vector_positive_axis", "z")),
           "slope_critical": float(need(slope, "critical_value", "SlopeFilter")),
           "step_critical": float(need(step, "critical_value", "Step filter")),
           "step_radius1": float(need(step, "first_window_radius", "Step filter")),
           "step_radius2": float(need(step, "second_window_radius", "Step filter")),
           "step_ncrit": int(need(step, "critical_cell_number", "Step filter")),
           "rough_critical": float(need(rough, "critical_value", "Roughness filter")),
           "rough_radius": float(need(rough, "estimation_radius", "Roughness filter"))})
    for d, dflt in ((slope, "traversability_slope"), (step, "traversability_step"), (rough, "traversability_roughness")):
        if str(d.get("map_type", dflt)) != dflt:
            raise ParamsYamlError(f"map_type must stay '{dflt}': the footprint checks read the layers by these names (TraversabilityMap.cpp:52-56)")
    if str(comb.get("output_layer", "traversability")) != "traversability":
        raise ParamsYamlError("MathExpressionFilter: output_layer must be 'traversability'")
    text = str(need(comb, "expression", "MathExpressionFilter"))
    try:
        out.update({k: float(v) for k, v in parse_weighted_sum(text).items()})
    except ParamsYamlError:
        if not general_expression:
            raise
    deleted = set()
    if len(chain) == 6:
        deleted = {str(s) for s in (prm[5].get("layers") or [])}
        extra = deleted - {"surface_normal_x", "surface_normal_y", "surface_normal_z"}
        if extra:
            raise ParamsYamlError(f"DeletionFilter: only the normal layers can be dropped (got {sorted(extra)})")
    out["keep_normals"] = len(deleted) != 3
    out["normals_algorithm"] = algorithm
    # criticalStepHeight_ of the footprint checks is the step filter's critical value (TraversabilityMap.cpp:104-111)
    out["fp_critical_step"] = out["step_critical"]
    return out


def footprint_fields(doc):
    fp = (doc or {}).get("footprint")
    if not isinstance(fp, dict):
        raise ParamsYamlError("no 'footprint' block in the footprint parameter file")
    out = {}
    if "circular_footprint_radius_inscribed" in fp:
        out["fp_radius"] = float(fp["circular_footprint_radius_inscribed"])  # radiusMin of traversabilityFootprint (:348)
    if "circular_footprint_offset" in fp:
        out["fp_offset"] = float(fp["circular_footprint_offset"])
    if "traversability_default" in fp:
        out["fp_default"] = float(fp["traversability_default"])
    if "verify_roughness_footprint" in fp:
        out["fp_check_roughness"] = 1 if fp["verify_roughness_footprint"] else 0
    return out


def robot_fields(doc):
    out = {}
    if isinstance(doc, dict) and "max_gap_width" in doc:
        out["fp_max_gap"] = float(doc["max_gap_width"])
    return out


def chain_expression(filter_yaml):
    """(text, is_weighted_sum): the MathExpressionFilter's expression as the file has it, and whether parse_weighted_sum
    accepts it -- te_run_chain's fused combine runs that form, te_run_expression any other."""
    doc = _load(filter_yaml)
    if not isinstance(doc, dict) or CHAIN_KEY not in doc:
        raise ParamsYamlError(f"no '{CHAIN_KEY}' list in the filter parameter file")
    found = [f for f in doc[CHAIN_KEY] if str(f.get("type")) == "gridMapFilters/MathExpressionFilter"]
    if len(found) != 1 or "expression" not in (found[0].get("params") or {}):
        raise ParamsYamlError("MathExpressionFilter did not find param expression")
    text = str(found[0]["params"]["expression"])
    try:
        parse_weighted_sum(text)
        return text, True
    except ParamsYamlError:
        return text, False


def fields_from_yaml(filter_yaml, footprint_yaml=None, robot_yaml=None, general_expression=False, normals_algorithm=False):
    """te_params fields + keep_normals.  normals_algorithm: also the key of that name (filter_chain_fields).  Without it a
    file that says `algorithm: raster` is refused -- the dict would describe the area method's chain -- and the key is left
    out: everything else in the dict is a field of te_params."""
    f = filter_chain_fields(_load(filter_yaml), general_expression)
    if not normals_algorithm:
        if f.pop("normals_algorithm"):
            raise ParamsYamlError("NormalVectorsFilter: algorithm: raster is an option of the context (TE_OPT_NORMALS_ALGORITHM), not a field "
                                  "of te_params: read the file with params_options_from_yaml")
    if footprint_yaml is not None:
        f.update(footprint_fields(_load(footprint_yaml)))
    if robot_yaml is not None:
        f.update(robot_fields(_load(robot_yaml)))
    return f


def params_from_yaml(capi, filter_yaml, footprint_yaml=None, robot_yaml=None):
    """(te_params validated by the library, run flags): the reference's files in, what te_set_params / te_run_chain take out."""
    f = fields_from_yaml(filter_yaml, footprint_yaml, robot_yaml)
    keep = f.pop("keep_normals")
    p = capi.default_params(**f)
    capi.validate_params(p)
    return p, (capi.RUN_KEEP_NORMALS if keep else 0)


def params_options_from_yaml(capi, filter_yaml, footprint_yaml=None, robot_yaml=None):
    """(te_params, run flags, options): params_from_yaml for a file that may say `algorithm: raster`.  options is a dict
    {option: value} for Context.set_option -- {capi.OPT_NORMALS_ALGORITHM: 0 | 1}."""
    f = fields_from_yaml(filter_yaml, footprint_yaml, robot_yaml, normals_algorithm=True)
    keep = f.pop("keep_normals")
    algorithm = f.pop("normals_algorithm")
    p = capi.default_params(**f)
    capi.validate_params(p)
    return p, (capi.RUN_KEEP_NORMALS if keep else 0), {capi.OPT_NORMALS_ALGORITHM: algorithm}


def params_and_expression_from_yaml(capi, filter_yaml, footprint_yaml=None, robot_yaml=None):
    """(te_params, run flags, text or None).  A weighted sum: what params_from_yaml gives, and None.  Any other expression: the
    params with the four weights at their defaults, and the text to hand to Context.run_expression behind run_chain (before
    run_footprint); the library's own compiler has accepted it (capi.expr_check raises TeError otherwise)."""
    text, weighted = chain_expression(filter_yaml)
    if weighted:
        p, flags = params_from_yaml(capi, filter_yaml, footprint_yaml, robot_yaml)
        return p, flags, None
    f = fields_from_yaml(filter_yaml, footprint_yaml, robot_yaml, general_expression=True)
    keep = f.pop("keep_normals")
    p = capi.default_params(**f)
    capi.validate_params(p)
    capi.expr_check(text)
    return p, (capi.RUN_KEEP_NORMALS if keep else 0), text


MEDIAN_FILL_TYPE = "gridMapFilters/MedianFillFilter"
_MEDIAN_FILL_KEYS = {"input_layer", "output_layer", "fill_hole_radius", "filter_existing_values", "existing_value_radius",
                     "num_erode_dilation_iterations", "fill_mask_layer", "debug"}


def median_fill_from_yaml(path_or_dict, resolution=None):
    """The settings of a `gridMapFilters/MedianFillFilter` entry -- the hole filling a grid_map pipeline puts in front of the
    chain -- or None when the file has none.  Looked for in every filter list of the document (a list of entries with `type`),
    `traversability_map_filters` among them; more than one entry is refused, and so is a key the filter does not have.  Keys
    and defaults as remembered from grid_map_filters (include/travgpu.h states the contract): fill_hole_radius 0.05,
    filter_existing_values false, existing_value_radius 0.0, num_erode_dilation_iterations 4; input_layer is required,
    output_layer defaults to it.  `fill_mask_layer` and `debug` are accepted and dropped: every call computes its mask, and
    the debug layers are not built.  With `resolution` the two radii also come in cells (`fill_hole_cells`,
    `existing_value_cells`: int(radius / resolution), the filter's own truncation).
    The dict's four parameters are the fields of capi.default_median_fill_params(**...)."""
    doc = path_or_dict if isinstance(path_or_dict, (dict, list)) else _load(path_or_dict)
    lists = [doc] if isinstance(doc, list) else [v for v in (doc or {}).values() if isinstance(v, list)]
    found = [f for lst in lists for f in lst if isinstance(f, dict) and str(f.get("type")) == MEDIAN_FILL_TYPE]
    if not found:
        return None
    if len(found) > 1:
        raise ParamsYamlError(f"{len(found)} MedianFillFilter entries: one fill in front of the chain is what is built")
    prm = found[0].get("params") or {}
    unknown = set(prm) - _MEDIAN_FILL_KEYS
    if unknown:
        raise ParamsYamlError(f"MedianFillFilter: unknown parameter(s) {sorted(unknown)}")
    if "input_layer" not in prm:
        raise ParamsYamlError("MedianFillFilter did not find param input_layer")
    out = {"input_layer": str(prm["input_layer"]), "output_layer": str(prm.get("output_layer", prm["input_layer"])),
           "fill_hole_radius": float(prm.get("fill_hole_radius", 0.05)),
           "filter_existing_values": 1 if prm.get("filter_existing_values", False) else 0,
           "existing_value_radius": float(prm.get("existing_value_radius", 0.0)),
           "num_erode_dilation_iterations": int(prm.get("num_erode_dilation_iterations", 4))}
    for k in ("fill_hole_radius", "existing_value_radius"):
        if not (np.isfinite(out[k]) and out[k] >= 0.0):
            raise ParamsYamlError(f"MedianFillFilter: {k} must be finite and not negative (got {out[k]})")
    if out["num_erode_dilation_iterations"] < 0:
        raise ParamsYamlError("MedianFillFilter: num_erode_dilation_iterations must not be negative")
    if resolution is not None:
        if not (np.isfinite(resolution) and resolution > 0.0):
            raise ParamsYamlError(f"resolution must be positive (got {resolution})")
        out["fill_hole_cells"] = int(out["fill_hole_radius"] / resolution)
        out["existing_value_cells"] = int(out["existing_value_radius"] / resolution)
    return out


WINDOW_EXPRESSION_TYPE = "gridMapFilters/SlidingWindowMathExpressionFilter"
_WINDOW_EXPRESSION_KEYS = {"input_layer", "output_layer", "expression", "window_size", "window_length", "compute_empty_cells", "edge_handling"}
_EDGE_HANDLING = ("inside", "crop", "empty", "mean")


def window_expression_from_yaml(path_or_dict):
    """The `gridMapFilters/SlidingWindowMathExpressionFilter` entries of every filter list of the document, in the order of the
    file: a list of dicts {"expression", "input_layer", "output_layer", "params": {"window_size" | "window_length",
    "compute_empty_cells", "edge_handling"}} -- "params" holds the arguments of capi.window_expr_params, the rest those of
    capi.Context.run_window_expression -- empty when the file has none.  An entry that cannot be honoured is refused whole: a key
    the filter does not have, a missing layer or expression, both or neither of window_size and window_length, an even or
    non-positive window_size, a length that is negative or not finite, an edge_handling that is none of the four (the
    contract: include/travgpu.h).  The expression itself is checked by capi.window_expr_check, which needs the library."""
    doc = path_or_dict if isinstance(path_or_dict, (dict, list)) else _load(path_or_dict)
    lists = [doc] if isinstance(doc, list) else [v for v in (doc or {}).values() if isinstance(v, list)]
    out = []
    name = "SlidingWindowMathExpressionFilter"
    for f in (f for lst in lists for f in lst if isinstance(f, dict) and str(f.get("type")) == WINDOW_EXPRESSION_TYPE):
        prm = f.get("params") or {}
        unknown = set(prm) - _WINDOW_EXPRESSION_KEYS
        if unknown:
            raise ParamsYamlError(f"{name}: unknown parameter(s) {sorted(unknown)}")
        for k in ("input_layer", "output_layer", "expression"):
            if k not in prm:
                raise ParamsYamlError(f"{name} did not find param {k}")
        if ("window_size" in prm) == ("window_length" in prm):
            raise ParamsYamlError(f"{name}: exactly one of window_size and window_length")
        params = {}
        if "window_size" in prm:
            w = prm["window_size"]
            if isinstance(w, bool) or not isinstance(w, int) or w < 1 or w % 2 == 0:
                raise ParamsYamlError(f"{name}: window_size must be an odd integer, at least 1 (got {w!r})")
            params["window_size"] = w
        else:
            length = float(prm["window_length"])
            if not (np.isfinite(length) and length >= 0.0):
                raise ParamsYamlError(f"{name}: window_length must be finite and not negative (got {length})")
            params["window_length"] = length
        empty = prm.get("compute_empty_cells", True)
        if not isinstance(empty, bool):
            raise ParamsYamlError(f"{name}: compute_empty_cells must be true or false (got {empty!r})")
        params["compute_empty_cells"] = empty
        edge = str(prm.get("edge_handling", "inside"))
        if edge not in _EDGE_HANDLING:
            raise ParamsYamlError(f"{name}: edge_handling must be one of {', '.join(_EDGE_HANDLING)} (got {edge!r})")
        params["edge_handling"] = edge
        if not str(prm["expression"]).strip():
            raise ParamsYamlError(f"{name}: the expression is empty")
        out.append({"expression": str(prm["expression"]), "input_layer": str(prm["input_layer"]), "output_layer": str(prm["output_layer"]),
                    "params": params})
    return out


RADIUS_FILTER_TYPES = {"gridMapFilters/MeanInRadiusFilter": "mean", "gridMapFilters/MinInRadiusFilter": "min"}
_RADIUS_FILTER_KEYS = {"radius", "input_layer", "output_layer"}


def radius_filter_from_yaml(path_or_dict):
    """The `gridMapFilters/MeanInRadiusFilter` and `gridMapFilters/MinInRadiusFilter` entries of every filter list of the
    document, in the order of the file: a list of dicts {"op": "mean" | "min", "radius", "input_layer", "output_layer"} -- the
    arguments of capi.Context.run_radius_filter -- empty when the file has none.  All three keys are required, as the
    filters' configure() has them (restated from grid_map_filters: include/travgpu.h); a key the filter does not have is
    refused, and so is a radius that is not finite or negative."""
    doc = path_or_dict if isinstance(path_or_dict, (dict, list)) else _load(path_or_dict)
    lists = [doc] if isinstance(doc, list) else [v for v in (doc or {}).values() if isinstance(v, list)]
    out = []
    for f in (f for lst in lists for f in lst if isinstance(f, dict) and str(f.get("type")) in RADIUS_FILTER_TYPES):
        name = str(f["type"]).split("/")[1]
        prm = f.get("params") or {}
        unknown = set(prm) - _RADIUS_FILTER_KEYS
        if unknown:
            raise ParamsYamlError(f"{name}: unknown parameter(s) {sorted(unknown)}")
        for k in ("radius", "input_layer", "output_layer"):
            if k not in prm:
                raise ParamsYamlError(f"{name} did not find param {k}")
        radius = float(prm["radius"])
        if not (np.isfinite(radius) and radius >= 0.0):
            raise ParamsYamlError(f"{name}: radius must be finite and not negative (got {radius})")
        out.append({"op": RADIUS_FILTER_TYPES[str(f["type"])], "radius": radius, "input_layer": str(prm["input_layer"]),
                    "output_layer": str(prm["output_layer"])})
    return out
