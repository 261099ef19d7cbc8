"""Guard bands around the device buffers a test hands to the library (plain torch: CPU and GPU tensors alike).

The contract every device entry is held to: bytes outside an operand never influence a result, bytes outside an output are never
written, inputs are never modified.  guarded() frames a buffer with `band` bytes of 0xFF on each side -- a NaN in fp16, fp32 and
fp64, -1 in the integer types -- so a load past an operand that is masked by arithmetic, not by a select, turns the result into NaN,
and a store past an output changes a byte that bands_intact() looks at.  What the bands cannot see: an over-read whose value a select
discards, and anything farther than `band` bytes away."""
import torch

BAND = 4096
_FILL = 0xFF


def guarded(shape, dtype, device, fill=None, band=BAND):
    """-> (buf, payload).  buf: flat uint8, band + nbytes + band bytes, every byte 0xFF.  payload: a view of the middle in `dtype` and
    `shape` (payload.data_ptr() == buf.data_ptr() + band), holding a copy of `fill` if one is given (the form for inputs)."""
    if band <= 0 or band % 256:
        raise ValueError(f"band must be a positive multiple of 256 bytes (alignment of the payload), got {band}")
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
    n = 1
    for s in shape:
        n *= s
    nbytes = n * torch.empty((), dtype=dtype).element_size()
    buf = torch.full((band + nbytes + band,), _FILL, dtype=torch.uint8, device=device)
    payload = buf[band:band + nbytes].view(dtype).view(shape)
    assert payload.data_ptr() == buf.data_ptr() + band and payload.is_contiguous()
    if fill is not None:
        if tuple(fill.shape) != shape or fill.dtype != dtype:
            raise ValueError(f"fill is {tuple(fill.shape)} {fill.dtype}, the payload {shape} {dtype}")
        payload.copy_(fill)
    return buf, payload


def bands_intact(buf, payload, band=BAND):
    """True iff every byte of both bands is still 0xFF.  Bytes are compared (no isnan): a kernel that writes a NaN into a band is seen."""
    nbytes = payload.numel() * payload.element_size()
    assert buf.dtype == torch.uint8 and buf.numel() == band + nbytes + band and payload.data_ptr() == buf.data_ptr() + band
    return bool((buf[:band] == _FILL).all()) and bool((buf[band + nbytes:] == _FILL).all())


def unchanged(payload, original):
    """Bitwise equality of an input with what was put into it (NaN payloads and the sign of zero included)."""
    if tuple(payload.shape) != tuple(original.shape) or payload.dtype != original.dtype:
        return False
    a = payload.detach().contiguous().reshape(-1).view(torch.uint8)
    b = original.detach().to(payload.device).contiguous().reshape(-1).view(torch.uint8)
    return bool(torch.equal(a, b))


class Guards:
    """The guarded buffers of one call: inp() / out() hand out payloads, check() asserts the contract for all of them."""

    def __init__(self, device, band=BAND):
        self.device, self.band, self.items = device, band, []

    def inp(self, t):
        orig = t.detach().contiguous().to(self.device, copy=True)     # kept on the payload's device: one upload, the comparison stays there
        buf, p = guarded(orig.shape, orig.dtype, self.device, fill=orig, band=self.band)
        self.items.append((buf, p, orig))
        return p

    def out(self, shape, dtype=torch.float32):
        buf, p = guarded(shape, dtype, self.device, band=self.band)
        self.items.append((buf, p, None))
        return p

    def check(self):
        for i, (buf, p, orig) in enumerate(self.items):
            assert bands_intact(buf, p, self.band), f"guard band of buffer {i} {tuple(p.shape)} {p.dtype} was written"
            if orig is not None:
                assert unchanged(p, orig), f"input {i} {tuple(p.shape)} {p.dtype} was modified"
