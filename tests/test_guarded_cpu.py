"""The detector detects: tests/guarded.py on the CPU, with torch CPU ops standing in for kernels.  Every negative case here fails
when the check it names is taken out of guarded.py."""
import pytest
import torch

from guarded import GUARD_BYTE, guarded

DTYPES = [torch.float32, torch.float16, torch.bfloat16]


def test_views_are_contiguous_aligned_and_prepoisoned():
    orig = torch.empty
    with guarded("cpu") as G:
        a = torch.empty(5, 7, dtype=torch.float16)
        b = torch.empty((3, 96), dtype=torch.float32, device="cpu")
        c = torch.empty_like(b)
        d = torch.empty(11, dtype=torch.uint8)
        e = torch.empty(4, dtype=torch.int32)
        assert torch.empty is not orig
    for t, shape in ((a, (5, 7)), (b, (3, 96)), (c, (3, 96)), (d, (11,)), (e, (4,))):
        assert tuple(t.shape) == shape and t.is_contiguous() and t.data_ptr() % 256 == 0
    assert a.isnan().all() and b.isnan().all() and c.isnan().all() and (d == 255).all() and (e == -1).all()
    assert len(G.allocs) == 5 and G.intact()
    for al in G.allocs:                      # guard | payload | pad | guard, guards of at least 4096 B / 32 rows, filled 0xA5
        assert al.start >= 4096 and al.buf.numel() - al.start - al.nbytes >= 4096
        assert (al.buf[:al.start] == GUARD_BYTE).all() and (al.buf[al.start + al.nbytes:] == GUARD_BYTE).all()
    with guarded("cpu") as G:
        wide = torch.empty(2, 3072, dtype=torch.float32)
    assert G.allocs[0].start >= 32 * 3072 * 4 and wide.data_ptr() % 256 == 0      # wide rows: 32 of them


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", ["front", "back"])
def test_one_element_overrun_is_reported(side, dtype):
    with guarded("cpu") as G:
        out = torch.empty(6, 10, dtype=dtype)
        out.fill_(1.0)                                                   # the stand-in kernel's legitimate stores
        assert G.intact()
        # ... and one element too far, through a view that reaches outside the payload
        off = out.storage_offset() - 1 if side == "front" else out.storage_offset() + out.numel()
        torch.as_strided(out, (1,), (1,), off).fill_(2.0)
        rep = G.intact()
    assert not rep
    text = repr(rep)
    assert side in text and "#0" in text and ("offset -1" in text if side == "front" else f"offset {out.numel() * out.element_size()}" in text), text


def test_overrun_into_the_16_byte_pad_is_reported():
    with guarded("cpu") as G:
        out = torch.empty(3, dtype=torch.uint8)
        torch.as_strided(out, (1,), (1,), out.storage_offset() + 3).fill_(0)
        assert not G.intact()


@pytest.mark.parametrize("dtype", DTYPES)
def test_unwritten_element_shows(dtype):
    with guarded("cpu") as G:
        out = torch.empty(4, 9, dtype=dtype)
        out[:, :8] = torch.ones(4, 8, dtype=dtype)                      # a stand-in that drops its tail column
    assert out[:, 8].isnan().all() and torch.isfinite(out[:, :8]).all()
    left = G.payload_left(out)
    assert left[:, 8].all() and not left[:, :8].any()
    rows = torch.zeros(4, dtype=torch.bool)
    rows[2] = True
    assert not G.untouched(out, rows)                                    # row 2 was (partly) written
    with guarded("cpu") as G:
        out = torch.empty(4, 9, dtype=dtype)
        out[~rows] = 3.0
    assert G.untouched(out, rows) and not G.untouched(out) and not G.untouched(out, ~rows)


def test_integer_and_byte_payload_pattern():
    with guarded("cpu") as G:
        idx = torch.empty(5, dtype=torch.int32)
        img = torch.empty(2, 8, dtype=torch.uint8)
        idx[:4] = torch.arange(4, dtype=torch.int32)
        img[0] = 7
    assert G.payload_left(idx).tolist() == [False] * 4 + [True]
    assert G.untouched(img, torch.tensor([False, True])) and not G.untouched(img, torch.tensor([True, False]))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("side", ["front", "back"])
def test_over_read_of_a_wrapped_input_poisons_the_result(side, dtype):
    x = torch.arange(1, 13, dtype=torch.float32).reshape(3, 4).to(dtype)
    with guarded("cpu") as G:
        w = G.wrap(x, name="x")
        assert torch.equal(w, x) and w.is_contiguous() and w.data_ptr() % 256 == 0
        good = torch.as_strided(w, (12,), (1,), w.storage_offset()).float().sum()
        off = w.storage_offset() - (side == "front")
        bad = torch.as_strided(w, (13,), (1,), off).float().sum()        # a stand-in that sums one element too many
        assert G.intact()                                                # reading does not disturb the guards
    assert float(good) == 78.0 and bad.isnan()


def test_integer_wraps_have_zero_guards_and_byte_images_0xff():
    with guarded("cpu") as G:
        m = G.wrap(torch.tensor([[3, 1], [2, 0]], dtype=torch.int32))
        m64 = G.wrap(torch.tensor([5, 6], dtype=torch.int64))
        img = G.wrap(torch.tensor([1, 2, 3], dtype=torch.uint8))
        f = G.wrap(torch.ones(2, 2))
        for t, n in ((m, 4), (m64, 2)):
            around = torch.as_strided(t, (n + 64,), (1,), t.storage_offset() - 32)
            assert (around[:32] == 0).all() and (around[32 + n:] == 0).all()     # an over-read index names element 0: never a wild address
        around = torch.as_strided(img, (3 + 32,), (1,), img.storage_offset() - 16)
        assert (around[:16] == 255).all() and (around[19:] == 255).all()
        assert torch.as_strided(f, (1,), (1,), f.storage_offset() + 4).isnan().all()
        assert G.wrap(torch.ones(2), poison="zero").dtype == torch.float32
        assert G.intact()
        torch.as_strided(m, (1,), (1,), m.storage_offset() + 4).fill_(9)         # a store behind an integer wrap is still seen
        assert not G.intact()


def test_originals_are_restored_after_an_exception():
    orig, orig_like = torch.empty, torch.empty_like
    with pytest.raises(ZeroDivisionError):
        with guarded("cpu"):
            assert torch.empty is not orig and torch.empty_like is not orig_like
            1 / 0
    assert torch.empty is orig and torch.empty_like is orig_like
    assert torch.empty(3).shape == (3,)


def test_pass_through_for_other_devices_and_keywords():
    with guarded("cpu") as G:
        meta = torch.empty(4, 4, device="meta")
        pinned_kw = torch.empty(8, dtype=torch.float32, pin_memory=False)
        grad_kw = torch.empty(8, requires_grad=False)
        fmt = torch.empty((1, 2, 3, 4), memory_format=torch.channels_last)
        like_kw = torch.empty_like(torch.zeros(2, 3, 4, 5), memory_format=torch.contiguous_format)
        like_strided = torch.empty_like(torch.zeros(4, 6).t())
        like_meta = torch.empty_like(torch.zeros(3, device="meta"))
        assert len(G.allocs) == 0
        assert meta.device.type == "meta" and like_meta.device.type == "meta" and pinned_kw.shape == grad_kw.shape == (8,)
        assert fmt.is_contiguous(memory_format=torch.channels_last) and like_kw.shape == (2, 3, 4, 5) and like_strided.shape == (6, 4)
    with guarded("cuda") as G:                                           # a CUDA registry leaves CPU allocations alone
        t = torch.empty(16)
        assert len(G.allocs) == 0 and t.shape == (16,)


def test_registry_keeps_dropped_buffers_alive_until_checked():
    with guarded("cpu") as G:
        def launch():
            ws = torch.empty(64, dtype=torch.uint8)                      # scratch dropped right after the "launch"
            torch.as_strided(ws, (1,), (1,), ws.storage_offset() + 64).fill_(0)
        launch()
        assert len(G.allocs) == 1 and not G.intact()


def test_other_payload_byte():
    with guarded("cpu", payload=0x00) as G:
        out = torch.empty(4, dtype=torch.uint8)
        out[:2] = 255
    assert out.tolist() == [255, 255, 0, 0] and G.payload_left(out).tolist() == [False, False, True, True]
