"""Self-test of tests/guards.py on CPU tensors: the helper the GPU tests rely on must itself notice every kind of damage."""
import pytest
import torch

from guards import BAND, Guards, bands_intact, guarded, unchanged

DTYPES = [torch.float16, torch.float32, torch.float64, torch.int32, torch.uint8]


@pytest.mark.parametrize("dtype", DTYPES, ids=[str(d).split(".")[1] for d in DTYPES])
def test_layout_and_offset(dtype):
    buf, p = guarded((3, 5), dtype, "cpu")
    nbytes = 15 * p.element_size()
    assert buf.dtype == torch.uint8 and buf.numel() == BAND + nbytes + BAND
    assert p.dtype == dtype and tuple(p.shape) == (3, 5) and p.is_contiguous()
    assert p.data_ptr() == buf.data_ptr() + BAND
    assert bool((buf == 0xFF).all())
    if dtype.is_floating_point:
        assert bool(torch.isnan(p).all())          # 0xFF bytes are a NaN in every float format used here
    elif dtype == torch.int32:
        assert bool((p == -1).all())
    assert bands_intact(buf, p)
    buf2, p2 = guarded((3, 5), dtype, "cpu", band=256)
    assert p2.data_ptr() == buf2.data_ptr() + 256 and buf2.numel() == 512 + nbytes and bands_intact(buf2, p2, band=256)


def test_untouched_buffer_passes_and_payload_writes_do_not_count():
    buf, p = guarded((7, 3), torch.float32, "cpu")
    assert bands_intact(buf, p)
    p.fill_(1.5)                                   # writing the payload, first and last element included, leaves the bands alone
    assert bands_intact(buf, p)
    assert bool((buf[:BAND] == 0xFF).all()) and bool((buf[BAND + 84:] == 0xFF).all())


@pytest.mark.parametrize("where", ["first", "last"])
def test_one_byte_in_the_front_band(where):
    buf, p = guarded((4,), torch.float32, "cpu")
    buf[0 if where == "first" else BAND - 1] = 0xFE
    assert not bands_intact(buf, p)


@pytest.mark.parametrize("where", ["first", "last"])
def test_one_byte_in_the_tail_band(where):
    buf, p = guarded((4,), torch.float32, "cpu")
    buf[BAND + 16 if where == "first" else BAND + 16 + BAND - 1] = 0x00
    assert not bands_intact(buf, p)


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32, torch.float64])
@pytest.mark.parametrize("side", ["front", "tail"])
def test_a_nan_written_into_a_band_is_seen(dtype, side):
    """The canonical NaN (0x7FC00000 in fp32) is not the 0xFF pattern: an isnan() check would pass it, the byte comparison does not."""
    buf, p = guarded((4,), dtype, "cpu")
    es = p.element_size()
    band = buf[:BAND] if side == "front" else buf[BAND + 4 * es:]
    as_float = band.view(dtype)
    as_float[BAND // es - 1 if side == "front" else 0] = float("nan")
    assert bool(torch.isnan(as_float).all())
    assert not bands_intact(buf, p)


def test_fill_and_unchanged():
    src = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    src[1, 1] = float("nan")
    src[2, 2] = -0.0
    buf, p = guarded(src.shape, src.dtype, "cpu", fill=src)
    assert unchanged(p, src) and bands_intact(buf, p)
    p[2, 2] = 0.0                                  # -0.0 -> +0.0: equal as numbers, different bits
    assert not unchanged(p, src)
    p[2, 2] = -0.0
    assert unchanged(p, src)
    p[0, 0] = 1.0
    assert not unchanged(p, src)
    ints = torch.tensor([[1, -2], [3, 4]], dtype=torch.int32)
    ibuf, ip = guarded(ints.shape, ints.dtype, "cpu", fill=ints)
    assert unchanged(ip, ints)
    ip[1, 1] += 1
    assert not unchanged(ip, ints)
    assert not unchanged(ip, ints.to(torch.int64))          # another dtype is never "unchanged"
    with pytest.raises(ValueError):
        guarded((2, 2), torch.float32, "cpu", fill=ints)


@pytest.mark.parametrize("band", [0, -256, 100, 4095, 4097, 128])
def test_band_must_be_a_multiple_of_256(band):
    with pytest.raises(ValueError):
        guarded((4,), torch.float32, "cpu", band=band)


def test_guards_collection():
    g = Guards("cpu")
    x = torch.randn(5, 3)
    xin = g.inp(x)
    out = g.out((5, 2))
    idx = g.out((4,), torch.int32)
    out.copy_(xin[:, :2])
    idx.zero_()
    g.check()
    xin[0, 0] += 1.0
    with pytest.raises(AssertionError, match="modified"):
        g.check()
    xin[0, 0] = x[0, 0]
    g.check()
    g.items[1][0][BAND + 40] = 0                   # the byte behind the [5, 2] fp32 output
    with pytest.raises(AssertionError, match="guard band"):
        g.check()
