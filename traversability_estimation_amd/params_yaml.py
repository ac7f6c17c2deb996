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


# ---- a grid_map_filters chain file as a list of steps (Context.run_filter_chain runs them) -------------------------------------
REFERENCE_LAYERS = ("elevation", "traversability_slope", "traversability_step", "traversability_roughness", "traversability",
                    "traversability_footprint", "surface_normal_x", "surface_normal_y", "surface_normal_z", "slope_footprint",
                    "step_footprint", "roughness_footprint", "traversability_x", "traversability_rot", "robot_slope")
_NORMAL_LAYERS = ("surface_normal_x", "surface_normal_y", "surface_normal_z")
_LAYER_NAME = re.compile(r"[A-Za-z_][A-Za-z0-9_]{0,62}\Z")
MAX_FUSED_THRESHOLDS = 4
_CHAIN_KEYS = {
    "NormalVectorsFilter": {"input_layer", "output_layers_prefix", "radius", "normal_vector_positive_axis", "algorithm", "parallelization_enabled",
                            "thread_number"},
    "SlopeFilter": {"map_type", "critical_value"},
    "StepFilter": {"map_type", "critical_value", "first_window_radius", "second_window_radius", "critical_cell_number"},
    "RoughnessFilter": {"map_type", "critical_value", "estimation_radius"},
    "MathExpressionFilter": {"output_layer", "expression"},
    "ThresholdFilter": {"layer", "condition_layer", "output_layer", "lower_threshold", "upper_threshold", "set_to"},
    "DuplicationFilter": {"input_layer", "output_layer"},
    "DeletionFilter": {"layers"},
}
_PLUGIN_MAP_TYPE = {"SlopeFilter": "traversability_slope", "StepFilter": "traversability_step", "RoughnessFilter": "traversability_roughness"}
_CHAIN_TYPES = ("MedianFillFilter", "MeanInRadiusFilter", "MinInRadiusFilter", "NormalVectorsFilter", "SlopeFilter", "StepFilter", "RoughnessFilter",
                "MathExpressionFilter", "SlidingWindowMathExpressionFilter", "ThresholdFilter", "DuplicationFilter", "DeletionFilter")


def _chain_step(entry, k):
    """One entry of a chain list as a step; every refusal names the entry."""
    name = str(entry.get("name", "entry %d" % k)) if isinstance(entry, dict) else "entry %d" % k

    def refuse(msg):
        raise ParamsYamlError(f"filter '{name}': {msg}")

    if not isinstance(entry, dict) or "type" not in entry:
        refuse("no type")
    ns, _, kind = str(entry["type"]).partition("/")
    if ns not in ("gridMapFilters", "traversabilityFilters") or kind not in _CHAIN_TYPES:
        refuse(f"type '{entry['type']}' is not built (built: {', '.join(_CHAIN_TYPES)})")
    prm = entry.get("params") or {}
    if not isinstance(prm, dict):
        refuse("params is not a map")
    one = [{"type": "gridMapFilters/" + kind, "params": prm}]
    try:  # the three readers this module already has: their checks, their words
        if kind == "MedianFillFilter":
            f = median_fill_from_yaml(one)
            return {"name": name, "filter": "median_fill", "input_layer": f.pop("input_layer"), "output_layer": f.pop("output_layer"), "params": f}
        if kind in ("MeanInRadiusFilter", "MinInRadiusFilter"):
            return dict(radius_filter_from_yaml(one)[0], name=name, filter="radius")
        if kind == "SlidingWindowMathExpressionFilter":
            return dict(window_expression_from_yaml(one)[0], name=name, filter="window_expression")
    except ParamsYamlError as e:
        refuse(str(e))
    unknown = set(prm) - _CHAIN_KEYS[kind]
    if unknown:
        refuse(f"{kind}: unknown parameter(s) {sorted(unknown)}")

    def need(key):
        if key not in prm:
            refuse(f"{kind} did not find param {key}")
        return prm[key]

    def number(key):
        try:
            v = float(need(key))
        except (TypeError, ValueError):
            refuse(f"{kind}: {key} must be a number (got {prm[key]!r})")
        if not np.isfinite(v):
            refuse(f"{kind}: {key} must be finite (got {v})")
        return v

    def layer(key):
        v = str(need(key))
        if not _LAYER_NAME.match(v):
            refuse(f"{kind}: {key} '{v}' is no layer name ([A-Za-z_][A-Za-z0-9_]*, at most 63 characters)")
        return v

    if kind == "NormalVectorsFilter":
        if str(prm.get("input_layer", "elevation")) != "elevation":
            refuse("NormalVectorsFilter: input_layer must be 'elevation' (the plugin reads the elevation layer)")
        if str(prm.get("output_layers_prefix", "surface_normal_")) != "surface_normal_":
            refuse("NormalVectorsFilter: output_layers_prefix must be 'surface_normal_' (SlopeFilter.cpp:71 hard-codes it)")
        algorithm = str(prm.get("algorithm", "area"))
        if algorithm not in ("area", "raster"):
            refuse(f"NormalVectorsFilter: algorithm must be area or raster (got '{algorithm}')")
        fields = {}
        if algorithm == "area" or "radius" in prm:
            fields["normals_radius"] = number("radius")
        try:
            fields["normals_axis"] = _axis(prm.get("normal_vector_positive_axis", "z"))
        except ParamsYamlError as e:
            refuse(str(e))
        return {"name": name, "filter": "normals", "fields": fields, "algorithm": algorithm}
    if kind in _PLUGIN_MAP_TYPE:
        want = _PLUGIN_MAP_TYPE[kind]
        if str(prm.get("map_type", want)) != want:
            refuse(f"{kind}: map_type must stay '{want}': the plugin writes the layer of that name")
        if kind == "SlopeFilter":
            fields = {"slope_critical": number("critical_value")}
        elif kind == "StepFilter":
            n = need("critical_cell_number")
            if isinstance(n, bool) or not isinstance(n, int):
                refuse(f"StepFilter: critical_cell_number must be an integer (got {n!r})")
            fields = {"step_critical": number("critical_value"), "step_radius1": number("first_window_radius"),
                      "step_radius2": number("second_window_radius"), "step_ncrit": n}
            fields["fp_critical_step"] = fields["step_critical"]
        else:
            fields = {"rough_critical": number("critical_value"), "rough_radius": number("estimation_radius")}
        return {"name": name, "filter": kind[:-len("Filter")].lower(), "fields": fields}
    if kind == "MathExpressionFilter":
        text = str(need("expression"))
        if not text.strip():
            refuse("MathExpressionFilter: the expression is empty")
        return {"name": name, "filter": "expression", "expression": text, "output_layer": layer("output_layer")}
    if kind == "ThresholdFilter":
        lower, upper = "lower_threshold" in prm, "upper_threshold" in prm
        if lower == upper:
            refuse("ThresholdFilter: exactly one of lower_threshold and upper_threshold (got %s)" % ("both" if lower else "neither"))
        names = {str(prm[k]) for k in ("layer", "condition_layer", "output_layer") if k in prm}
        if not names:
            refuse("ThresholdFilter did not find param layer")
        if len(names) > 1:
            refuse(f"ThresholdFilter: the filter runs in place: layer, condition_layer and output_layer must name one layer (got {sorted(names)})")
        key = "layer" if "layer" in prm else "condition_layer" if "condition_layer" in prm else "output_layer"
        return {"name": name, "filter": "threshold", "layer": layer(key), "mode": "lower" if lower else "upper",
                "threshold": number("lower_threshold" if lower else "upper_threshold"), "set_to": float(need("set_to"))}
    if kind == "DuplicationFilter":
        return {"name": name, "filter": "duplication", "input_layer": layer("input_layer"), "output_layer": layer("output_layer")}
    layers = need("layers")
    if not isinstance(layers, list) or not layers:
        refuse("DeletionFilter: layers must be a list of layer names")
    layers = [str(v) for v in layers]
    kept = [v for v in layers if v in REFERENCE_LAYERS and v not in _NORMAL_LAYERS]
    if kept:
        refuse(f"DeletionFilter: {kept} are layers of the context itself and cannot be deleted (the normal layers are dropped, user layers removed)")
    return {"name": name, "filter": "deletion", "layers": layers}


def filter_chain_from_yaml(path_or_text, key=None):
    """A grid_map_filters chain file as the list of steps Context.run_filter_chain runs, in file order.  `key`: the name of the
    list in the document (default: `traversability_map_filters` if it is there, otherwise the document's only list; a document
    that IS a list needs none).  Types, as gridMapFilters/... or traversabilityFilters/...: MedianFillFilter, MeanInRadiusFilter,
    MinInRadiusFilter, NormalVectorsFilter (area or raster), SlopeFilter, StepFilter, RoughnessFilter, MathExpressionFilter,
    SlidingWindowMathExpressionFilter, ThresholdFilter, DuplicationFilter, DeletionFilter.  Every key each filter reads is
    checked; any other type, an unknown key and a ThresholdFilter with both or neither threshold raise ParamsYamlError with the
    entry's name.  A step is a dict with "name", "filter" and that filter's arguments; the three plugins and NormalVectorsFilter
    carry the te_params fields their entry sets ("fields"): they run as te_run_filter on the reference's layer names."""
    doc = _load(path_or_text)
    if isinstance(doc, list):
        chain = doc
    else:
        lists = {k: v for k, v in (doc or {}).items() if isinstance(v, list)} if isinstance(doc, dict) else {}
        if key is None:
            key = CHAIN_KEY if CHAIN_KEY in lists else next(iter(lists)) if len(lists) == 1 else None
        if key is None or key not in lists:
            raise ParamsYamlError(f"no filter list {'named ' + repr(key) if key else 'to choose'} in the chain file (lists: {sorted(lists)})")
        chain = lists[key]
    if not chain:
        raise ParamsYamlError("the filter list is empty")
    return [_chain_step(e, k) for k, e in enumerate(chain)]


def plan_filter_chain(steps, fuse=True):
    """The steps grouped into the calls the runner issues: a list of (call, step, extra).  With `fuse` a MathExpressionFilter
    takes the ThresholdFilters that DIRECTLY follow it on its output layer into its own launch
    (te_run_layer_expression_thresholds), at most MAX_FUSED_THRESHOLDS of them: a threshold on another layer, or behind any
    other filter, is a call of its own, and so is the fifth threshold and every one behind it."""
    out, k = [], 0
    while k < len(steps):
        s = steps[k]
        k += 1
        if s["filter"] != "expression":
            out.append((s["filter"], s, None))
            continue
        fused = []
        while fuse and k < len(steps) and len(fused) < MAX_FUSED_THRESHOLDS and steps[k]["filter"] == "threshold" and steps[k]["layer"] == s["output_layer"]:
            fused.append(steps[k])
            k += 1
        out.append(("expression", s, fused))
    return out
