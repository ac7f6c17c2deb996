"""Reference evaluator of the MathExpressionFilter language of te_run_expression, written from the contract in
include/travgpu.h (not from csrc/te_expr.h): a recursive-descent parser that evaluates as it goes, in numpy float32.

    evaluate(text, layers) -> float32 array of the layers' shape

`layers`: name -> float32 array [batch, cols, rows] (or [batch, n]); every array the same shape.  Every operation rounds to
float32.  Reductions are taken per map of the batch (axis 0) through math.fsum, i.e. the exactly rounded float64 sum, and are
rounded to float32 at the end.  The transcendental functions and ^ are the float64 numpy function of the float32 argument
rounded to float32 -- the reference the GPU tests measure the device's functions against.

Errors: ExprError with .kind "BAD_PARAM" (not an expression of the language) or "UNSUPPORTED" (valid EigenLab, not built).
Limits of the compiled form (instruction count, stack depth) are the library's own and are not modelled here.
"""
import math
import re

import numpy as np

LAYER_NAMES = ("elevation", "traversability_slope", "traversability_step", "traversability_roughness", "traversability",
               "traversability_footprint", "surface_normal_x", "surface_normal_y", "surface_normal_z", "slope_footprint",
               "step_footprint", "roughness_footprint", "traversability_x", "traversability_rot", "robot_slope")
_NUMBER = re.compile(r"(?:\d+(?:\.(?![*/^])\d*)?|\.\d+)(?:[eE][-+]?\d+)?")
_NAME = re.compile(r"[A-Za-z_][A-Za-z_0-9]*")
_UNSUPPORTED = {"min", "max", "transpose", "trace", "norm", "zeros", "ones", "eye"}
_REDUCTIONS = {"sum", "mean", "sumOfFinites", "meanOfFinites", "minOfFinites", "maxOfFinites", "numberOfFinites"}


class ExprError(ValueError):
    def __init__(self, kind, msg):
        super().__init__(f"{kind}: {msg}")
        self.kind = kind


def _f64(fn):
    def f(x):
        with np.errstate(all="ignore"):
            return fn(x.astype(np.float64)).astype(np.float32)
    return f


_UNARY = {"abs": np.abs, "sqrt": lambda x: np.sqrt(x), "square": lambda x: x * x, "exp": _f64(np.exp), "log": _f64(np.log),
          "log10": _f64(np.log10), "sin": _f64(np.sin), "cos": _f64(np.cos), "tan": _f64(np.tan), "asin": _f64(np.arcsin),
          "acos": _f64(np.arccos)}


def _fsum(values):
    try:
        return math.fsum(values)
    except (ValueError, OverflowError):  # inf - inf, or an intermediate overflow
        return float(np.sum(np.asarray(values, dtype=np.float64)))


class _Parser:
    def __init__(self, text, layers):
        self.s, self.i, self.layers = text, 0, layers
        self.shape = next(iter(layers.values())).shape
        self.in_reduction = False

    # a node is (is_map, float32 array); a scalar has shape [batch, 1, ...] so that it broadcasts per map
    def scalar(self, v):
        return False, np.full((self.shape[0],) + (1,) * (len(self.shape) - 1), v, dtype=np.float32)

    def ws(self):
        while self.i < len(self.s) and self.s[self.i] in " \t\r\n":
            self.i += 1

    def peek(self, *tokens):
        self.ws()
        for t in tokens:
            if self.s.startswith(t, self.i):
                return t
        return None

    def take(self, *tokens):
        t = self.peek(*tokens)
        if t:
            self.i += len(t)
        return t

    def top(self):
        self.ws()
        if self.i >= len(self.s):
            raise ExprError("BAD_PARAM", "empty expression")
        node = self.expr()
        self.ws()
        if self.i < len(self.s):
            c = self.s[self.i]
            raise ExprError("UNSUPPORTED" if c in "=<>~!&|'[]:;" else "BAD_PARAM", f"unexpected '{c}' at {self.i}")
        return node

    def expr(self):
        a = self.term()
        while True:
            op = self.take("+", "-")
            if not op:
                return a
            b = self.term()
            with np.errstate(all="ignore"):
                a = (a[0] or b[0], (a[1] + b[1]) if op == "+" else (a[1] - b[1]))

    def term(self):
        a = self.unary()
        while True:
            op = self.take(".*", "./", "*", "/")
            if not op:
                return a
            b = self.unary()
            if op == "*" and a[0] and b[0]:
                raise ExprError("UNSUPPORTED", "map * map is the matrix product; write .*")
            with np.errstate(all="ignore"):
                a = (a[0] or b[0], (a[1] * b[1]) if op in ("*", ".*") else (a[1] / b[1]))

    def unary(self):
        op = self.take("-", "+")
        if op:
            a = self.unary()
            return (a[0], -a[1]) if op == "-" else a
        return self.power()

    def power(self):
        a = self.primary()
        while True:
            op = self.take(".^", "^")
            if not op:
                return a
            neg = False
            while True:
                sign = self.take("-", "+")
                if not sign:
                    break
                neg ^= sign == "-"
            b = self.primary()
            if neg:
                b = (b[0], -b[1])
            if op == "^" and b[0]:
                raise ExprError("UNSUPPORTED", "^ needs a scalar exponent; write .^")
            with np.errstate(all="ignore"):
                x, y = np.broadcast_arrays(a[1].astype(np.float64), b[1].astype(np.float64))
                a = (a[0] or b[0], np.power(x, y).astype(np.float32))

    def close(self):
        if not self.take(")"):
            raise ExprError("BAD_PARAM", f"')' expected at {self.i}")

    def primary(self):
        self.ws()
        m = _NUMBER.match(self.s, self.i)
        if m:
            self.i = m.end()
            if self.i < len(self.s) and (self.s[self.i].isalpha() or self.s[self.i] == "_"):
                raise ExprError("BAD_PARAM", f"unexpected character behind a number at {self.i}")
            return self.scalar(np.float32(float(m.group(0))))
        if self.take("("):
            a = self.expr()
            self.close()
            return a
        m = _NAME.match(self.s, self.i)
        if not m:
            raise ExprError("UNSUPPORTED" if self.peek("[") else "BAD_PARAM", f"operand expected at {self.i}")
        name = m.group(0)
        self.i = m.end()
        if name in LAYER_NAMES:
            if self.peek("("):
                raise ExprError("UNSUPPORTED", "indexing")
            if name not in self.layers:
                raise KeyError(name)
            return True, np.asarray(self.layers[name], dtype=np.float32)
        if name in _UNSUPPORTED:
            raise ExprError("UNSUPPORTED", name)
        if name not in _UNARY and name not in _REDUCTIONS and name not in ("cwiseMin", "cwiseMax"):
            raise ExprError("BAD_PARAM", f"unknown name {name}")
        if not self.take("("):
            raise ExprError("BAD_PARAM", f"'(' expected behind {name}")
        if name in _REDUCTIONS:
            if self.in_reduction:
                raise ExprError("BAD_PARAM", "reductions do not nest")
            self.in_reduction = True
            a = self.expr()
            self.in_reduction = False
            self.close()
            return self.reduce(name, a)
        a = self.expr()
        if name in _UNARY:
            self.close()
            with np.errstate(all="ignore"):
                return a[0], np.asarray(_UNARY[name](a[1]), dtype=np.float32)
        if not self.take(","):
            raise ExprError("BAD_PARAM", f"{name} takes two arguments")
        b = self.expr()
        self.close()
        x, y = np.broadcast_arrays(a[1], b[1])
        with np.errstate(all="ignore"):
            # std::min(a, b) = (b < a) ? b : a; std::max(a, b) = (a < b) ? b : a -- a NaN in a is returned, one in b dropped
            return a[0] or b[0], np.where(y < x, y, x) if name == "cwiseMin" else np.where(x < y, y, x)

    def reduce(self, name, a):
        full = np.broadcast_to(a[1], self.shape).reshape(self.shape[0], -1)
        out = np.empty(self.shape[0], dtype=np.float32)
        for m in range(self.shape[0]):
            v = full[m].astype(np.float64)
            fin = v[np.isfinite(v)]
            with np.errstate(all="ignore"):
                if name == "sum":
                    r = _fsum(v)
                elif name == "mean":
                    r = _fsum(v) / v.size
                elif name == "sumOfFinites":
                    r = _fsum(fin)
                elif name == "meanOfFinites":
                    r = _fsum(fin) / fin.size if fin.size else float("nan")
                elif name == "minOfFinites":
                    r = fin.min() if fin.size else float("nan")
                elif name == "maxOfFinites":
                    r = fin.max() if fin.size else float("nan")
                else:
                    r = float(fin.size)
                out[m] = np.float32(r)
        return False, out.reshape((self.shape[0],) + (1,) * (len(self.shape) - 1))


def evaluate(text, layers):
    p = _Parser(str(text), layers)
    _, v = p.top()
    return np.ascontiguousarray(np.broadcast_to(v, p.shape), dtype=np.float32)


def same_bits(a, b):
    """Equal float32 bit patterns, every NaN counting as the same value (a NaN's payload is not part of the contract)."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and bool(np.array_equal(na, nb)) and bool(np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def ulp_distance(a, b):
    """Largest distance in float32 units in the last place over the cells where neither is NaN (NaN positions must agree)."""
    a, b = np.asarray(a, dtype=np.float32).ravel(), np.asarray(b, dtype=np.float32).ravel()
    na = np.isnan(a)
    assert np.array_equal(na, np.isnan(b)), "NaN positions differ"
    def key(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    d = np.abs(key(a[~na]) - key(b[~na]))
    return int(d.max()) if d.size else 0
