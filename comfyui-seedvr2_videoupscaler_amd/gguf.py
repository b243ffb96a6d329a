"""GGUF (llama.cpp / ComfyUI-GGUF block-quantised) checkpoints: reader, the specification of the expansion, loader, a small writer.

A GGUF weight IS, here, the format's canonical fp32 dequantisation rounded once to bf16 (nearest even); F32 / F16 / BF16 tensors
keep their dtype exactly as a safetensors tensor would.  The file is read once, every quantised tensor is expanded once -- on the
device by csrc/svr_gguf.hip where the backend has ``dequant_gguf`` (HipOps), by ``dequantize_torch`` below otherwise -- and the
engines receive the state dict a safetensors file would have produced: weights resident as bf16, no quantised execution.

``dequantize_torch`` is the specification of the kernels, bit for bit.  ``e`` is the element index inside a block, ``l = e % 32``;
``d`` / ``dmin`` are IEEE fp16; everything is little-endian; all arithmetic in fp32:

  Q8_0   34 B / 32     d | int8 q[32]                             x[e] = d * q[e]
  Q4_K   144 B / 256   d | dmin | scales[12] | qs[128]            x[e] = (d * sc[j]) * q[e] - dmin * m[j],  j = e // 32,
                       q[e] the low (j even) / high (j odd) nibble of qs[32 (e // 64) + l];  six-bit sc[j], m[j]:
                       j < 4:  sc = scales[j] & 63                               m = scales[j + 4] & 63
                       j >= 4: sc = (scales[j + 4] & 15) | (scales[j - 4] >> 6 << 4)   m = (scales[j + 4] >> 4) | (scales[j] >> 6 << 4)
  Q5_K   176 B / 256   d | dmin | scales[12] | qh[32] | qs[128]   as Q4_K with bit j of qh[l] as the fifth bit of q[e] (0..31)
  Q6_K   210 B / 256   ql[128] | qh[64] | int8 scales[16] | d     x[e] = (d * scales[e // 16]) * (q[e] - 32),  h = e // 128,
                       r = (e % 128) // 32: the low (r < 2) / high (r >= 2) nibble of ql[64 h + 32 (r & 1) + l] with bits 2r, 2r + 1
                       of qh[32 h + l] above it

d * sc * q is exact in fp32 (an fp16 significand has 11 bits, the sub-scale at most 7, the quant at most 5: 23 <= 24), so the one
subtraction of Q4_K / Q5_K is the only rounding, an FMA contraction changes nothing, and the values equal the reference's own block
functions evaluated in fp32 (src/optimization/gguf_dequant.py; its runtime route evaluates the same expressions in fp16 -- its own
precision loss).  The expression order (d * sc) * q - (dmin * m) fixes the sign of a zero.  Scales are not validated: an inf / NaN
fp16 scale gives inf / NaN weights, and the engines' finite guards speak.

File format (little-endian): ``GGUF`` | u32 version (2, 3) | u64 tensor_count | u64 kv_count | key-value pairs | tensor infos |
padding to ``general.alignment`` (u32, default 32) | data.  A tensor info is name | u32 n_dims | u64 ne[n_dims] | u32 type | u64
offset into the data region; ne[0] varies fastest, so the torch shape is reversed(ne) -- or ``comfy.gguf.orig_shape.<name>`` (an
i32 array) where a converter flattened the tensor to quantise it (model_loader.py:228-239).
"""
import mmap
import os
import struct
from typing import Any, Dict, List, NamedTuple, Optional, Tuple

import torch

MAGIC = b"GGUF"
DEFAULT_ALIGNMENT = 32
F32, F16, Q8_0, Q4_K, Q5_K, Q6_K, BF16 = 0, 1, 8, 12, 13, 14, 30
# ggml type id -> (name, elements per block, bytes per block, torch dtype of a plain type | None for a quantised one)
TYPES = {
    F32: ("F32", 1, 4, torch.float32),
    F16: ("F16", 1, 2, torch.float16),
    BF16: ("BF16", 1, 2, torch.bfloat16),
    Q8_0: ("Q8_0", 32, 34, None),
    Q4_K: ("Q4_K", 256, 144, None),
    Q5_K: ("Q5_K", 256, 176, None),
    Q6_K: ("Q6_K", 256, 210, None),
}
QUANTISED = tuple(t for t, v in TYPES.items() if v[3] is None)
# the ids this loader does not expand, by name, so that a refusal says which table entry and kernel case are missing
OTHER_TYPE_NAMES = {2: "Q4_0", 3: "Q4_1", 6: "Q5_0", 7: "Q5_1", 9: "Q8_1", 10: "Q2_K", 11: "Q3_K", 15: "Q8_K", 16: "IQ2_XXS",
                    17: "IQ2_XS", 18: "IQ3_XXS", 19: "IQ1_S", 20: "IQ4_NL", 21: "IQ3_S", 22: "IQ2_S", 23: "IQ4_XS", 24: "I8",
                    25: "I16", 26: "I32", 27: "I64", 28: "F64", 29: "IQ1_M", 34: "TQ1_0", 35: "TQ2_0", 39: "MXFP4"}
# metadata value types
U8, I8, U16, I16, U32, I32, FLOAT32, BOOL, STRING, ARRAY, U64, I64, FLOAT64 = range(13)
_SCALAR = {U8: "<B", I8: "<b", U16: "<H", I16: "<h", U32: "<I", I32: "<i", FLOAT32: "<f", BOOL: "<?", U64: "<Q", I64: "<q",
           FLOAT64: "<d"}
STAGING_BYTES = 64 << 20          # one pinned staging piece of the device route (two are in flight)


def type_name(ggml_type: int) -> str:
    if ggml_type in TYPES:
        return TYPES[ggml_type][0]
    return OTHER_TYPE_NAMES.get(ggml_type, f"ggml type {ggml_type}")


class TensorInfo(NamedTuple):
    name: str
    ggml_type: int
    shape: Tuple[int, ...]        # logical torch shape: reversed(ne) or comfy.gguf.orig_shape.<name>
    ne: Tuple[int, ...]           # the file's extents, fastest first
    offset: int                   # of the first byte, from the start of the FILE
    nbytes: int
    data: torch.Tensor            # uint8 [nbytes]: a view of the memory-mapped file


# ---------------------------------------------------------------------------------------------------------------- specification
def _as_blocks(blocks: torch.Tensor, ggml_type: int) -> torch.Tensor:
    if ggml_type not in QUANTISED:
        raise ValueError(f"dequantize: unsupported ggml type {type_name(ggml_type)} (supported: "
                         f"{', '.join(TYPES[t][0] for t in QUANTISED)})")
    size = TYPES[ggml_type][2]
    if blocks.dtype != torch.uint8 or blocks.numel() == 0 or blocks.numel() % size:
        raise ValueError(f"dequantize: {type_name(ggml_type)} blocks must be uint8 with a multiple of {size} bytes, got "
                         f"{blocks.dtype} {tuple(blocks.shape)}")
    return blocks.reshape(-1, size)


def _half(b: torch.Tensor, at: int) -> torch.Tensor:
    """the fp16 at byte ``at`` of every block, as fp32 [n, 1]"""
    return b[:, at:at + 2].contiguous().view(torch.float16).float()


def _k_scales_mins(scales: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """[n, 12] bytes -> the eight six-bit scales and the eight six-bit mins, fp32 [n, 8] each"""
    s = scales.to(torch.int32)
    sc = [s[:, j] & 63 for j in range(4)] + [(s[:, j + 4] & 15) | ((s[:, j - 4] >> 6) << 4) for j in range(4, 8)]
    m = [s[:, j + 4] & 63 for j in range(4)] + [(s[:, j + 4] >> 4) | ((s[:, j] >> 6) << 4) for j in range(4, 8)]
    return torch.stack(sc, dim=1).float(), torch.stack(m, dim=1).float()


def dequantize_torch(blocks: torch.Tensor, ggml_type: int, out_dtype: torch.dtype = torch.bfloat16) -> torch.Tensor:
    """uint8 blocks (any shape holding whole blocks) of a quantised type -> [n_blocks, block size] in fp32, or rounded to bf16.  Any
    device.  The statement the kernels of csrc/svr_gguf.hip are equal to, bit for bit."""
    if out_dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"dequantize: out_dtype must be torch.float32 or torch.bfloat16, got {out_dtype}")
    b = _as_blocks(blocks, ggml_type)
    dev = b.device
    if ggml_type == Q8_0:
        x = _half(b, 0) * b[:, 2:34].contiguous().view(torch.int8).float()
    elif ggml_type in (Q4_K, Q5_K):
        e = torch.arange(256, device=dev)
        j, l = e // 32, e % 32
        sc, m = _k_scales_mins(b[:, 4:16])
        qs_at = 16 if ggml_type == Q4_K else 48
        byte = b[:, qs_at + 32 * (e // 64) + l].to(torch.int32)
        q = torch.where(j % 2 == 1, byte >> 4, byte & 15)
        if ggml_type == Q5_K:
            q = q | (((b[:, 16 + l].to(torch.int32) >> j) & 1) << 4)
        x = (_half(b, 0) * sc)[:, j] * q.float() - (_half(b, 2) * m)[:, j]
    else:
        e = torch.arange(256, device=dev)
        h, r, l = e // 128, (e % 128) // 32, e % 32
        low = b[:, 64 * h + 32 * (r & 1) + l].to(torch.int32)
        low = torch.where(r >= 2, low >> 4, low & 15)
        high = (b[:, 128 + 32 * h + l].to(torch.int32) >> (2 * r)) & 3
        q = (low | (high << 4)) - 32
        x = (_half(b, 208) * b[:, 192:208].contiguous().view(torch.int8).float())[:, e // 16] * q.float()
    return x if out_dtype == torch.float32 else x.to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------- reader
class _Cursor:
    def __init__(self, buf, path):
        self.buf, self.path, self.at = buf, path, 0

    def take(self, fmt):
        try:
            (v,) = struct.unpack_from(fmt, self.buf, self.at)
        except struct.error:
            raise ValueError(f"{self.path}: the file ends inside its header (at byte {self.at})") from None
        self.at += struct.calcsize(fmt)
        return v

    def string(self):
        n = self.take("<Q")
        if self.at + n > len(self.buf):
            raise ValueError(f"{self.path}: the file ends inside its header (a string of {n} bytes at byte {self.at})")
        s = bytes(self.buf[self.at:self.at + n])
        self.at += n
        return s.decode("utf-8", errors="replace")

    def value(self, vtype):
        if vtype in _SCALAR:
            return self.take(_SCALAR[vtype])
        if vtype == STRING:
            return self.string()
        if vtype == ARRAY:
            etype, n = self.take("<I"), self.take("<Q")
            if etype in _SCALAR and etype != BOOL:          # (one unpack for a long numeric array)
                fmt = "<" + str(n) + _SCALAR[etype][1]
                try:
                    vals = list(struct.unpack_from(fmt, self.buf, self.at))
                except struct.error:
                    raise ValueError(f"{self.path}: the file ends inside its header (an array of {n} at byte {self.at})") from None
                self.at += struct.calcsize(fmt)
                return vals
            return [self.value(etype) for _ in range(n)]
        raise ValueError(f"{self.path}: unknown metadata value type {vtype} at byte {self.at}")


def _open(path: str):
    """-> (mmap, metadata, tensor infos).  Every failure is a ValueError naming the path."""
    try:
        with open(path, "rb") as f:
            size = os.fstat(f.fileno()).st_size
            if size < 24:
                raise ValueError(f"{path}: not a GGUF file ({size} bytes: shorter than the header)")
            # (private copy-on-write pages: torch wants a writable buffer for a zero-copy view; nothing is ever written)
            mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_COPY)
    except OSError as e:
        raise ValueError(f"{path}: cannot read the GGUF file: {e}") from None
    if mm[:4] != MAGIC:
        raise ValueError(f"{path}: not a GGUF file (magic {bytes(mm[:4])!r}, expected {MAGIC!r})")
    cur = _Cursor(mm, path)
    cur.at = 4
    version = cur.take("<I")
    if version not in (2, 3):
        swapped = struct.unpack(">I", struct.pack("<I", version))[0]
        if swapped in (2, 3):
            raise ValueError(f"{path}: big-endian GGUF file (version {swapped} byte-swapped); only little-endian files are read")
        raise ValueError(f"{path}: unsupported GGUF version {version} (versions 2 and 3 are read)")
    n_tensors, n_kv = cur.take("<Q"), cur.take("<Q")
    metadata: Dict[str, Any] = {}
    for _ in range(n_kv):
        key = cur.string()
        metadata[key] = cur.value(cur.take("<I"))
    raw = []
    for _ in range(n_tensors):
        name = cur.string()
        n_dims = cur.take("<I")
        if n_dims > 8:
            raise ValueError(f"{path}: tensor {name!r} has {n_dims} dimensions")
        ne = tuple(cur.take("<Q") for _ in range(n_dims))
        raw.append((name, ne, cur.take("<I"), cur.take("<Q")))
    alignment = metadata.get("general.alignment", DEFAULT_ALIGNMENT)
    if not isinstance(alignment, int) or isinstance(alignment, bool) or alignment < 1:
        raise ValueError(f"{path}: general.alignment is {alignment!r}")
    data_start = (cur.at + alignment - 1) // alignment * alignment
    whole = torch.frombuffer(mm, dtype=torch.uint8) if size else None
    infos, seen = [], set()
    for name, ne, ggml_type, rel in raw:
        if name in seen:
            raise ValueError(f"{path}: duplicate tensor name {name!r}")
        seen.add(name)
        if ggml_type not in TYPES:
            raise ValueError(f"{path}: tensor {name!r} has the unsupported ggml type {type_name(ggml_type)} (id {ggml_type}; "
                             f"supported: {', '.join(v[0] for v in TYPES.values())})")
        tname, per, bsize, _ = TYPES[ggml_type]
        numel = 1
        for n in ne:
            numel *= n
        if ne and ne[0] % per:
            raise ValueError(f"{path}: tensor {name!r} ({tname}): ne[0] = {ne[0]} is not a multiple of the block size {per}")
        nbytes = numel // per * bsize
        start = data_start + rel
        if start + nbytes > size:
            raise ValueError(f"{path}: tensor {name!r} ({tname}, {nbytes} bytes at {start}) runs past the end of the file ({size} bytes)")
        shape = tuple(reversed(ne))
        logical = metadata.get(f"comfy.gguf.orig_shape.{name}")
        if isinstance(logical, list) and all(isinstance(n, int) for n in logical):
            count = 1
            for n in logical:
                count *= n
            if count != numel:
                raise ValueError(f"{path}: tensor {name!r} ({tname}): comfy.gguf.orig_shape {logical} does not hold its {numel} elements")
            shape = tuple(logical)
        infos.append(TensorInfo(name, ggml_type, shape, ne, start, nbytes, whole[start:start + nbytes]))
    return mm, metadata, infos


def read_gguf(path: str) -> Tuple[Dict[str, Any], List[TensorInfo]]:
    """(metadata, tensor infos) of a GGUF file over a memory map: ``info.data`` is a uint8 view of the tensor's bytes in the mapped
    file (pages come in when they are touched; the file is never read as a whole).  Raises ValueError naming the path."""
    _, metadata, infos = _open(path)
    return metadata, infos


# ---------------------------------------------------------------------------------------------------------------- loader
def _plain(raw: torch.Tensor, info: TensorInfo) -> torch.Tensor:
    """bytes of an F32 / F16 / BF16 tensor -> an owning tensor of that dtype and the logical shape"""
    return raw.clone().view(TYPES[info.ggml_type][3]).reshape(info.shape)


def _to_device_staged(mm, start: int, stop: int, device) -> torch.Tensor:
    """File bytes [start, stop) -> one uint8 device tensor, through two pinned staging pieces of STAGING_BYTES: the host fills one
    from the map while the other is in flight; an event per piece says when it may be refilled."""
    whole = torch.frombuffer(mm, dtype=torch.uint8)
    with torch.cuda.device(device):
        dev = torch.empty(stop - start, dtype=torch.uint8, device=device)
        piece = min(STAGING_BYTES, max(stop - start, 1))
        stage = [torch.empty(piece, dtype=torch.uint8).pin_memory() for _ in range(2)]
        busy = [None, None]
        for i, at in enumerate(range(start, stop, piece)):
            n = min(piece, stop - at)
            k = i % 2
            if busy[k] is not None:
                busy[k].synchronize()
            stage[k][:n].copy_(whole[at:at + n])
            dev[at - start:at - start + n].copy_(stage[k][:n], non_blocking=True)
            busy[k] = torch.cuda.Event()
            busy[k].record()
        for ev in busy:                               # (the pinned pieces go back to the host allocator: their copies must be done)
            if ev is not None:
                ev.synchronize()
    return dev


def load_state_dict(path: str, device="cpu", ops=None) -> Dict[str, torch.Tensor]:
    """name -> tensor, as a safetensors file of the same weights would give: quantised tensors expanded to bf16 (the fp32
    dequantisation rounded once), F32 / F16 / BF16 in their own dtype, logical shapes.
    ``ops`` with ``dequant_gguf`` (HipOps): the data region goes to ``ops.device`` through pinned staging pieces, every quantised
    tensor is expanded there by csrc/svr_gguf.hip on the current stream (no host synchronisation per tensor), the byte buffer is
    released and the tensors stay on the device; a failing library raises -- there is no fall-back from it.  Any other ``ops``, or
    none: ``dequantize_torch`` tensor by tensor on ``device``."""
    mm, _, infos = _open(path)
    out: Dict[str, torch.Tensor] = {}
    if ops is not None and hasattr(ops, "dequant_gguf"):
        if not infos:
            return out
        lo, hi = min(i.offset for i in infos), max(i.offset + i.nbytes for i in infos)
        buf = _to_device_staged(mm, lo, hi, ops.device)
        for info in infos:
            raw = buf[info.offset - lo:info.offset - lo + info.nbytes]
            if info.ggml_type in QUANTISED:
                out[info.name] = ops.dequant_gguf(raw, info.ggml_type, torch.bfloat16).reshape(info.shape)
            else:
                out[info.name] = _plain(raw, info)
        del buf, raw              # (stream-ordered: the allocator hands the bytes out again only behind the launches that read them)
        return out
    for info in infos:
        raw = info.data.to(device)
        if info.ggml_type in QUANTISED:
            out[info.name] = dequantize_torch(raw, info.ggml_type, torch.bfloat16).reshape(info.shape)
        else:
            out[info.name] = _plain(raw, info)
    return out


# ---------------------------------------------------------------------------------------------------------------- writer
def _pack_value(vtype: int, value) -> bytes:
    if vtype in _SCALAR:
        return struct.pack(_SCALAR[vtype], value)
    if vtype == STRING:
        raw = value.encode("utf-8")
        return struct.pack("<Q", len(raw)) + raw
    if vtype == ARRAY:
        etype, items = value
        return struct.pack("<IQ", etype, len(items)) + b"".join(_pack_value(etype, v) for v in items)
    raise ValueError(f"unknown metadata value type {vtype}")


def _typed(value):
    """(value type, value) for a metadata entry given without its type: bool, str, int (u32 when it fits, else i64), float (f32),
    a list of ints (array of i32) or of strs."""
    if isinstance(value, tuple):
        return value
    if isinstance(value, bool):
        return BOOL, value
    if isinstance(value, str):
        return STRING, value
    if isinstance(value, int):
        return (U32, value) if 0 <= value < 2 ** 32 else (I64, value)
    if isinstance(value, float):
        return FLOAT32, value
    if isinstance(value, list):
        return ARRAY, ((STRING if value and isinstance(value[0], str) else I32), value)
    raise ValueError(f"cannot infer a GGUF value type for {value!r}")


def write_gguf(path: str, tensors, metadata: Optional[Dict[str, Any]] = None, version: int = 3) -> None:
    """A GGUF file from READY-MADE data (tests and tools; the product only reads).  ``tensors``: an iterable of
    (name, ggml type, shape, data) -- ``shape`` the torch shape (written reversed), ``data`` a uint8 tensor of whole blocks for a
    quantised type, a tensor of the type's own dtype for F32 / F16 / BF16.  ``metadata``: key -> value or (value type, value), an
    array as (ARRAY, (element type, items)); ``general.alignment`` there sets the alignment of the data region and of every tensor."""
    metadata = dict(metadata or {})
    alignment = _typed(metadata.get("general.alignment", DEFAULT_ALIGNMENT))[1]
    head = bytearray(MAGIC + struct.pack("<IQQ", version, 0, len(metadata)))
    for key, value in metadata.items():
        vtype, v = _typed(value)
        head += _pack_value(STRING, key) + struct.pack("<I", vtype) + _pack_value(vtype, v)
    blobs, at, count = [], 0, 0
    for name, ggml_type, shape, data in tensors:
        tname, per, bsize, dtype = TYPES[ggml_type]
        numel = 1
        for n in shape:
            numel *= n
        raw = data.detach().cpu().contiguous()
        if dtype is not None and raw.dtype != dtype:
            raise ValueError(f"write_gguf: tensor {name!r} ({tname}) needs {dtype} data, got {raw.dtype}")
        raw = raw.reshape(-1).view(torch.uint8)
        if raw.numel() * per != numel * bsize:
            raise ValueError(f"write_gguf: tensor {name!r} ({tname}) of shape {tuple(shape)} needs {numel // per * bsize} bytes, got {raw.numel()}")
        head += _pack_value(STRING, name) + struct.pack("<I", len(shape)) + b"".join(struct.pack("<Q", n) for n in reversed(shape))
        head += struct.pack("<IQ", ggml_type, at)
        blobs.append((at, raw.numpy().tobytes()))
        at = (at + raw.numel() + alignment - 1) // alignment * alignment
        count += 1
    head[8:16] = struct.pack("<Q", count)
    data_start = (len(head) + alignment - 1) // alignment * alignment
    with open(path, "wb") as f:
        f.write(bytes(head))
        for rel, blob in blobs:
            f.write(b"\0" * (data_start + rel - f.tell()))
            f.write(blob)
