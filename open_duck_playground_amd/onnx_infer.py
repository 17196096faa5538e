"""ONNX policy inference on the host (mirror of playground/common/onnx_infer.py:4-24).

The reference runs the exported policy with onnxruntime's CPU provider; onnxruntime is not
installed here, so this module decodes the ONNX protobuf itself (a wire-format reader, no
generated classes) and evaluates the graph with numpy. It supports the operator set the policy
export emits (common/export_onnx.py via onnx_export.py: Sub, Div, Gemm, Sigmoid, Mul, Tanh, Relu,
Add, MatMul, Identity) and raises on anything else, so a graph it cannot run fails loudly.
"""

from __future__ import annotations

from typing import Dict, List, Tuple

import numpy as np


def _varint(b: bytes, i: int) -> Tuple[int, int]:
    shift = v = 0
    while True:
        c = b[i]
        i += 1
        v |= (c & 0x7F) << shift
        if c < 0x80:
            return v, i
        shift += 7


def _fields(b: bytes):
    """(field number, wire type, value) of one protobuf message; length-delimited values as bytes."""
    i, n = 0, len(b)
    while i < n:
        key, i = _varint(b, i)
        f, w = key >> 3, key & 7
        if w == 0:
            v, i = _varint(b, i)
        elif w == 2:
            ln, i = _varint(b, i)
            v, i = b[i:i + ln], i + ln
        elif w == 5:
            v, i = b[i:i + 4], i + 4
        elif w == 1:
            v, i = b[i:i + 8], i + 8
        else:
            raise ValueError(f"unsupported protobuf wire type {w}")
        yield f, w, v


def _tensor(b: bytes) -> Tuple[str, np.ndarray]:
    dims, dtype, name, raw, floats = [], 1, "", None, []
    for f, w, v in _fields(b):
        if f == 1:
            if w == 2:  # packed dims
                j = 0
                while j < len(v):
                    d, j = _varint(v, j)
                    dims.append(d)
            else:
                dims.append(v)
        elif f == 2:
            dtype = v
        elif f == 8:
            name = v.decode()
        elif f == 9:
            raw = v
        elif f == 4:  # float_data
            floats.append(np.frombuffer(v, "<f4") if w == 2 else np.frombuffer(v, "<f4"))
    if dtype != 1:
        raise ValueError(f"initializer {name}: only float32 tensors are supported")
    a = np.frombuffer(raw, "<f4") if raw is not None else np.concatenate(floats)
    return name, a.reshape(dims).astype(np.float32)


def _node(b: bytes):
    ins, outs, op, attrs = [], [], "", {}
    for f, _, v in _fields(b):
        if f == 1:
            ins.append(v.decode())
        elif f == 2:
            outs.append(v.decode())
        elif f == 4:
            op = v.decode()
        elif f == 5:  # AttributeProto: name 1, f 2, i 3
            an, av = "", None
            for g, w, x in _fields(v):
                if g == 1:
                    an = x.decode()
                elif g == 2:
                    av = float(np.frombuffer(x, "<f4")[0])
                elif g == 3:
                    av = x
            attrs[an] = av
    return op, ins, outs, attrs


class OnnxGraph:
    def __init__(self, blob: bytes):
        graph = next(v for f, _, v in _fields(blob) if f == 7)
        self.nodes: List[tuple] = []
        self.init: Dict[str, np.ndarray] = {}
        self.inputs: List[str] = []
        self.outputs: List[str] = []
        for f, _, v in _fields(graph):
            if f == 1:
                self.nodes.append(_node(v))
            elif f == 5:
                k, a = _tensor(v)
                self.init[k] = a
            elif f == 11:
                self.inputs.append(next(x.decode() for g, _, x in _fields(v) if g == 1))
            elif f == 12:
                self.outputs.append(next(x.decode() for g, _, x in _fields(v) if g == 1))

    def run(self, feeds: Dict[str, np.ndarray]) -> List[np.ndarray]:
        env = dict(self.init)
        env.update({k: np.asarray(v, dtype=np.float32) for k, v in feeds.items()})
        for op, ins, outs, attrs in self.nodes:
            x = [env[i] for i in ins]
            if op == "Sub":
                y = x[0] - x[1]
            elif op == "Div":
                y = x[0] / x[1]
            elif op == "Add":
                y = x[0] + x[1]
            elif op == "Mul":
                y = x[0] * x[1]
            elif op == "Gemm":
                a = x[0].T if attrs.get("transA") else x[0]
                b = x[1].T if attrs.get("transB") else x[1]
                y = attrs.get("alpha", 1.0) * (a @ b)
                if len(x) > 2:
                    y = y + attrs.get("beta", 1.0) * x[2]
            elif op == "MatMul":
                y = x[0] @ x[1]
            elif op == "Sigmoid":
                y = 1.0 / (1.0 + np.exp(-x[0]))
            elif op == "Tanh":
                y = np.tanh(x[0])
            elif op == "Relu":
                y = np.maximum(x[0], 0)
            elif op == "Identity":
                y = x[0]
            else:
                raise NotImplementedError(f"ONNX op {op} is not supported by onnx_infer")
            env[outs[0]] = y.astype(np.float32)
        return [env[o] for o in self.outputs]


def dense_policy(graph: OnnxGraph) -> Dict[str, object]:
    """The exported policy's graph as the arguments of ``duck_policy_act`` (include/duck_ppo.h), for the
    device-resident deployment loop (sim2sim.FleetInfer).

    Recognised: an optional ``Sub(mean)`` then ``Div(std)`` on the input; dense layers, each a ``Gemm``
    (``transB`` honoured) or a ``MatMul`` + ``Add``, with ``Sigmoid`` + ``Mul`` (swish) between them; a final
    ``Tanh`` on the graph's output. Anything else -- ``alpha`` / ``beta`` != 1, ``transA``, a tensor with
    another consumer, ``Relu``, a missing ``Tanh``, a stray node -- raises ValueError naming the node.

    Returns ``sizes`` [nlayers + 1], ``W[l]`` float32 in nn.Linear layout [out, in], ``b[l]`` [out], ``mean``
    and ``istd = float32(1 / float64(std))`` [sizes[0]] (both None without a normaliser). The file holds only
    the ``loc`` half of the output layer and duck_policy_act wants (loc | scale), so the last layer is
    zero-padded from A to 2A outputs: ``sizes[-1] == 2 A``."""
    nodes = graph.nodes

    def label(k):
        op, ins, outs, _ = nodes[k]
        return f"{op} node -> {outs[0]!r}"

    users: Dict[str, List[int]] = {}
    for k, (_, ins, _, _) in enumerate(nodes):
        for i in ins:
            users.setdefault(i, []).append(k)
    feeds = [i for i in graph.inputs if i not in graph.init]
    if len(feeds) != 1 or len(graph.outputs) != 1:
        raise ValueError(f"a policy graph has one input and one output, not {feeds} -> {graph.outputs}")
    seen = set()

    def only_user(x, what):
        """The one node that consumes tensor x."""
        u = users.get(x, [])
        if len(u) != 1 or x in graph.outputs:
            names = ", ".join(label(k) for k in u) or "no node"
            raise ValueError(f"{what} {x!r} must feed exactly one node, but feeds {names}")
        seen.add(u[0])
        return (u[0],) + tuple(nodes[u[0]])

    def const_operand(k, ins, x):
        """The initializer a binary node k combines x with, as its second operand."""
        if len(ins) != 2 or ins[0] != x or ins[1] not in graph.init:
            raise ValueError(f"{label(k)}: expected ({x!r}, initializer), got {ins}")
        return graph.init[ins[1]]

    x = feeds[0]
    mean = istd = None
    if [nodes[k][0] for k in users.get(x, [])] == ["Sub"]:
        k, _, ins, outs, _ = only_user(x, "input")
        mean = const_operand(k, ins, x)
        x = outs[0]
        k, op, ins, outs, _ = only_user(x, "centred input")
        if op != "Div":
            raise ValueError(f"{label(k)}: a Sub on the input must be followed by Div(std)")
        istd = (1.0 / const_operand(k, ins, x).astype(np.float64)).astype(np.float32)
        x = outs[0]
    Ws, bs = [], []
    while True:
        k, op, ins, outs, attrs = only_user(x, "layer input")
        if op == "Gemm":
            if len(ins) not in (2, 3) or ins[0] != x or any(i not in graph.init for i in ins[1:]):
                raise ValueError(f"{label(k)}: expected ({x!r}, kernel[, bias]) with initializers, got {ins}")
            if attrs.get("alpha", 1.0) != 1.0 or attrs.get("beta", 1.0) != 1.0 or attrs.get("transA"):
                raise ValueError(f"{label(k)}: alpha, beta != 1 and transA are not a dense layer")
            w = graph.init[ins[1]]
            w = w if attrs.get("transB") else w.T
            b = graph.init[ins[2]] if len(ins) == 3 else np.zeros(w.shape[0], np.float32)
            y = outs[0]
        elif op == "MatMul":
            w = const_operand(k, ins, x).T
            k2, op2, ins2, outs2, _ = only_user(outs[0], "MatMul output")
            if op2 != "Add":
                raise ValueError(f"{label(k2)}: a MatMul must be followed by Add(bias)")
            if ins2[0] != outs[0]:
                ins2 = ins2[::-1]   # bias + product
            b = const_operand(k2, ins2, outs[0])
            y = outs2[0]
        else:
            raise ValueError(f"{label(k)}: expected a Gemm or a MatMul")
        if w.ndim != 2 or b.reshape(-1).shape[0] != w.shape[0] or (Ws and w.shape[1] != Ws[-1].shape[0]):
            raise ValueError(f"{label(k)}: kernel {w.T.shape} and bias {b.shape} do not chain")
        Ws.append(np.ascontiguousarray(w, dtype=np.float32))
        bs.append(np.ascontiguousarray(b.reshape(-1), dtype=np.float32))
        after = users.get(y, [])
        ops = sorted(nodes[j][0] for j in after)
        if ops == ["Tanh"]:
            k, _, _, outs, _ = only_user(y, "last layer")
            if outs[0] != graph.outputs[0] or users.get(outs[0]):
                raise ValueError(f"{label(k)}: Tanh must produce the graph's output")
            break
        if ops != ["Mul", "Sigmoid"] or y in graph.outputs:
            names = ", ".join(label(j) for j in after) or "no node"
            raise ValueError(f"layer output {y!r} must feed Sigmoid and Mul (swish) or the final Tanh, but feeds {names}")
        ks = next(j for j in after if nodes[j][0] == "Sigmoid")
        km = next(j for j in after if nodes[j][0] == "Mul")
        sig = nodes[ks][2][0]
        if users.get(sig, []) != [km] or sorted(nodes[km][1]) != sorted([y, sig]):
            raise ValueError(f"{label(km)}: expected {y!r} * Sigmoid({y!r})")
        seen.update((ks, km))
        x = nodes[km][2][0]
    stray = [label(k) for k in range(len(nodes)) if k not in seen]
    if stray:
        raise ValueError(f"nodes outside the dense policy chain: {', '.join(stray)}")
    n_in = Ws[0].shape[1]
    if mean is not None:
        mean = np.ascontiguousarray(np.broadcast_to(mean.reshape(-1), (n_in,)), dtype=np.float32)
        istd = np.ascontiguousarray(np.broadcast_to(istd.reshape(-1), (n_in,)), dtype=np.float32)
    A = Ws[-1].shape[0]
    Ws[-1] = np.concatenate([Ws[-1], np.zeros_like(Ws[-1])], 0)
    bs[-1] = np.concatenate([bs[-1], np.zeros_like(bs[-1])], 0)
    return {"sizes": [n_in] + [w.shape[0] for w in Ws], "W": Ws, "b": bs, "mean": mean, "istd": istd,
            "action_size": A}


class OnnxInfer:
    """``OnnxInfer(onnx_model_path, input_name="obs", awd=False).infer(inputs)`` as in
    common/onnx_infer.py: with ``awd`` the input is one observation, fed as a batch of one."""

    def __init__(self, onnx_model_path: str, input_name: str = "obs", awd: bool = False):
        self.onnx_model_path = onnx_model_path
        with open(onnx_model_path, "rb") as f:
            self.graph = OnnxGraph(f.read())
        self.input_name = input_name
        self.awd = awd

    def infer(self, inputs):
        if self.awd:
            return self.graph.run({self.input_name: np.asarray([inputs], dtype=np.float32)})[0][0]
        return self.graph.run({self.input_name: np.asarray(inputs, dtype=np.float32)})[0]
