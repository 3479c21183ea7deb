"""rope_packed_at: RoPE on packed rows at shard positions (GPU). It shares
rope_rotate8 with the dense kernels, so a shard's rows must come out
bit-identical to the same rows of the full-sequence rope_packed result."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D = 128
S, HEADS, N_ROT = 8192, 4, 3
CHUNK = S // 8


@pytest.fixture(scope="module")
def full():
    """x [1,8192,4*128] and its rope_packed rotation of heads 0-2 (head 3
    plays v: never rotated). Shared, read-only."""
    from trainingjob_operator_amd.ops import make_inv_freq, native
    from trainingjob_operator_amd.ops.attention import _rope_packed
    g = torch.Generator(device=DEV).manual_seed(12)
    x = torch.randn(1, S, HEADS * D, device=DEV, generator=g).bfloat16()
    inv_freq = make_inv_freq(D, 500000.0, device=DEV)
    rot = x.clone()
    _rope_packed(native.load(require=True), x, rot, inv_freq, S, N_ROT,
                 HEADS * D, HEADS * D, S, D, 1.0)
    assert not torch.equal(rot[..., :N_ROT * D], x[..., :N_ROT * D])
    return x, rot, inv_freq


def _rows(chunks):
    return torch.cat([torch.arange(c * CHUNK, (c + 1) * CHUNK)
                      for c in chunks]).to(DEV)


def test_two_segment_shard_equals_rows_of_the_full_rotation(full):
    from trainingjob_operator_amd.ops.attention import rope_packed_at
    x, rot, inv_freq = full
    rows = _rows((1, 6))                  # the zig-zag shard of rank 1 of 4
    xs = x[:, rows].contiguous()
    out = torch.full((1, 2 * CHUNK, N_ROT * D), float("nan"),
                     dtype=torch.bfloat16, device=DEV)   # rot-only row width
    rope_packed_at(xs, out, inv_freq, N_ROT, 2 * CHUNK, CHUNK, 1 * CHUNK,
                   6 * CHUNK)
    assert torch.equal(out, rot[:, rows][..., :N_ROT * D])


def test_one_segment_at_an_offset(full):
    from trainingjob_operator_amd.ops.attention import rope_packed_at
    x, rot, inv_freq = full
    rows = _rows((3,))                    # pos_a = 3 * 1024
    xs = x[:, rows].contiguous()
    out = xs.clone()
    rope_packed_at(xs, out, inv_freq, N_ROT, CHUNK, CHUNK, 3 * CHUNK)
    assert torch.equal(out, rot[:, rows])         # v head copied untouched
    # batch of two shards: row s = t % S restarts per batch element
    xb = torch.cat([xs, xs], dim=0)
    outb = torch.empty_like(xb)[..., :N_ROT * D].contiguous()
    rope_packed_at(xb, outb, inv_freq, N_ROT, CHUNK, CHUNK, 3 * CHUNK)
    assert torch.equal(outb[1], rot[0, rows][..., :N_ROT * D])


def test_in_place_inverse_returns_the_input(full):
    from trainingjob_operator_amd.ops.attention import rope_packed_at
    x, _, inv_freq = full
    rows = _rows((1, 6))
    xs = x[:, rows].contiguous()
    buf = xs.clone()
    args = (inv_freq, N_ROT, 2 * CHUNK, CHUNK, 1 * CHUNK, 6 * CHUNK)
    rope_packed_at(buf, buf, *args, sign=1.0)
    assert not torch.equal(buf[..., :N_ROT * D], xs[..., :N_ROT * D])
    assert torch.equal(buf[..., N_ROT * D:], xs[..., N_ROT * D:])
    rope_packed_at(buf, buf, *args, sign=-1.0)
    assert torch.equal(buf[..., N_ROT * D:], xs[..., N_ROT * D:])
    # One bf16 step, at the pair's length r = |(x1, x2)|, which the rotation
    # keeps: the forward rounds each component by at most half a step of
    # r (2^-7 r bounds a step), the inverse turns that error vector (length
    # <= sqrt(2)/2 steps) back onto the axes and rounds once more (1/2):
    # at most (sqrt(2)/2 + 1/2) = 1.21 steps of 2^-7 r. Both directions use
    # the same sin/cos, so their own error cancels to fp32 precision.
    a, b = buf[..., :N_ROT * D].float(), xs[..., :N_ROT * D].float()
    r = b.view(1, -1, N_ROT, 2, D // 2).pow(2).sum(dim=3, keepdim=True).sqrt()
    step = (r * 2.0 ** -7).expand(-1, -1, -1, 2, -1).reshape(a.shape)
    err = (a - b).abs()
    print(f"round trip: max abs err {err.max().item():.5f}, "
          f"max err/step {(err / step).max().item():.3f}")
    assert bool((err <= 1.21 * step).all())


def test_bad_segments_and_positions_are_refused(full):
    from trainingjob_operator_amd.ops.attention import rope_packed_at
    x, _, inv_freq = full
    xs = x[:, :2 * CHUNK].contiguous()
    out = torch.full_like(xs, float("nan"))
    for seg_len, pos_a, pos_b in (
            (CHUNK + 8, 0, 0),            # S is neither seg_len nor 2*seg_len
            (3 * CHUNK, 0, 0),
            (0, 0, 0),
            (CHUNK, -1, 0),               # negative positions
            (CHUNK, 0, -5),
            (CHUNK, 2 ** 24 - CHUNK + 1, 0),   # past float-exact positions
            (CHUNK, 0, 2 ** 24)):
        with pytest.raises(RuntimeError):
            rope_packed_at(xs, out, inv_freq, N_ROT, 2 * CHUNK, seg_len,
                           pos_a, pos_b)
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all()), "a refused call launched"
    # the largest position still allowed
    rope_packed_at(xs, out, inv_freq, N_ROT, 2 * CHUNK, CHUNK,
                   2 ** 24 - CHUNK, 0)
    assert not bool(torch.isnan(out[..., :N_ROT * D]).any())
