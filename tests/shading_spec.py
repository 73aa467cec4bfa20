"""The compute shader's shading, restated in plain numpy: what a ray sees.

An independent reference for the arithmetic that no reference artifact pins:
random_in_unit_sphere, reflect, refract, the Schlick reflectance, the three
scatter branches and the RNG draws each consumes, the sky, the attenuation
product, "depth ran out -> black", CSMain's two-draw jitter and the
toGamma(sum / spp) finish. Written from ShaderCompute.hlsl and SURVEY.md (§7
"FXC semantics", Appendix A) alone, in this project's own words, with the HLSL
line of every formula beside it; it imports neither the oracle nor the GPU
library and was written without consulting their shading code. Its worth is
that independence: keep it that way.

What is exact and what is not
    The RNG is exact: the fp32 seed chain (seed += 0.1 twice per draw),
    baseHash on 32-bit integers, hash1 / hash2 / hash3 as the fp32 values the
    shader forms (divisors float(0xffffffffU) and float(0x7fffffff), which
    round to 2^32 and 2^31). Everything else runs in the float type `dtype`:
    np.float64 is the reference; np.float32 exists only to size a tolerance
    (how far an honest fp32 evaluation of the same text lies from fp64).
    HLSL literals are fp32 values first, as the shader compiler sees them
    (lit()).

Shape
    Every function works on a batch: vectors are (n, 3), scalars (n,), and the
    path loops advance all live paths in lockstep. A path that ended keeps its
    seed: draws are taken by the lanes that reach them and by no other.
    Functions are looked up in this module when called, so a test can replace
    one (a deliberate misreading) and see whether a check notices.

Not covered: the thin lens, per-sample RNG, frame_index seeds and
RTX_FRAME_LAMBERT_GUARD. These are this project's extensions and have no
compute-shader text to restate. Seeds are an input of trace(), so how a caller
derived them does not matter there.

Where the text is easy to misread (kept for the next reader)
    * :306-307 take u from the FIRST hash2's .x and v from the SECOND hash2's
      .y: two draws per sample, half of each thrown away.
    * :241 `cant || reflectance > hash1(p)`: SM5 `||` does not short-circuit,
      hash1 is drawn when cant is true too.
    * :232 the ratio is 1 / ir on the FRONT face; reflectance() is then called
      with that ratio, not with ir (:241).
    * :171 `root < t_min || t_max < root`: a root equal to the closest so far
      is accepted, so of two equal hits the later sphere wins.
    * :182 the normal is (p - c) / r with the signed radius.
    * :33 divides by float(0xffffffffU) = 2^32 but :40, :47 by
      float(0x7fffffff) = 2^31, after masking to 31 bits.
"""
import numpy as np

f32 = np.float32
u64 = np.uint64
M32 = u64(0xFFFFFFFF)
M31 = u64(0x7FFFFFFF)
K_HASH = u64(1103515245)
T_MIN = 0.001  # :262


def lit(x, dtype):
    """An HLSL literal: an fp32 value, then whatever the arithmetic runs in."""
    return dtype(f32(x))


# ---------------------------------------------------------------------------
# RNG: exact (:23-48)
# ---------------------------------------------------------------------------
def base_hash(px, py):
    """baseHash (:23-28) on 32-bit values held in uint64, wrapped by hand."""
    px, py = np.asarray(px, u64) & M32, np.asarray(py, u64) & M32
    qx = (K_HASH * ((px >> u64(1)) ^ py)) & M32   # :25, p = K * ((p >> 1) ^ p.yx), both lanes from the old p
    qy = (K_HASH * ((py >> u64(1)) ^ px)) & M32
    h = (K_HASH * (qx ^ (qy >> u64(3)))) & M32    # :26
    return h ^ (h >> u64(16))                     # :27


def _bits(x):
    return np.ascontiguousarray(x, f32).view(np.uint32).astype(u64)


def advance(seed):
    """`baseHash(asuint(float2(seed += 0.1, seed += 0.1)))` (:32, :38, :45), left
    to right: the hash word and the seed after the two additions."""
    a = (np.asarray(seed, f32) + f32(0.1)).astype(f32)
    b = (a + f32(0.1)).astype(f32)
    return base_hash(_bits(a), _bits(b)), b


def _unit(n, divisor):
    return (n.astype(f32) / f32(divisor)).astype(f32)  # float(uint): round to nearest, as astype does


def hash1(seed):
    """:30-34 -> (value, seed)."""
    n, seed = advance(seed)
    return _unit(n, 0xFFFFFFFF), seed


def hash2(seed):
    """:36-41 -> (x, y, seed)."""
    n, seed = advance(seed)
    return _unit(n & M31, 0x7FFFFFFF), _unit(((n * u64(48271)) & M32) & M31, 0x7FFFFFFF), seed


def hash3(seed):
    """:43-48 -> (x, y, z, seed)."""
    n, seed = advance(seed)
    return (_unit(n & M31, 0x7FFFFFFF), _unit(((n * u64(16807)) & M32) & M31, 0x7FFFFFFF),
            _unit(((n * u64(48271)) & M32) & M31, 0x7FFFFFFF), seed)


def pixel_seed(x, y):
    """:295, float(baseHash(DTid.xy)) / float(0xffffffffU)."""
    return _unit(base_hash(x, y), 0xFFFFFFFF)


# ---------------------------------------------------------------------------
# vectors (:59-97)
# ---------------------------------------------------------------------------
def dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def length(a):
    return np.sqrt(dot(a, a))


def normalize(a):
    return a / length(a)[..., None]


def col(s):
    return s[..., None]


def random_in_unit_sphere(seed, dtype):
    """:59-66 -> ((n, 3), seed). One hash3."""
    x, y, z, seed = hash3(seed)
    hx = x.astype(dtype) * lit(2.0, dtype) - lit(1.0, dtype)       # :61
    phi = y.astype(dtype) * lit(6.28318530718, dtype) - lit(0.0, dtype)
    hz = z.astype(dtype) * lit(1.0, dtype) - lit(0.0, dtype)
    r = np.power(hz, dtype(f32(1.0) / f32(3.0)))                   # :63, the quotient of two fp32 literals
    s = np.sqrt(lit(1.0, dtype) - hx * hx)                         # :65
    return col(r) * np.stack([s * np.sin(phi), s * np.cos(phi), hx], -1), seed


def reflect(v, n):
    """:76-79."""
    return v - col(lit(2.0, v.dtype.type) * dot(v, n)) * n


def refract(uv, n, ratio):
    """:81-88."""
    T = uv.dtype.type
    cos_theta = np.minimum(dot(-uv, n), lit(1.0, T))               # :83
    perp = col(ratio) * (uv + col(cos_theta) * n)                  # :84
    par = col(-np.sqrt(np.abs(lit(1.0, T) - length(perp) * length(perp)))) * n  # :85
    return perp + par


def reflectance(cosine, ref_idx):
    """:90-97, Schlick."""
    T = cosine.dtype.type
    r0 = (lit(1.0, T) - ref_idx) / (lit(1.0, T) + ref_idx)         # :93
    r0 = r0 * r0                                                   # :94
    return r0 + (lit(1.0, T) - r0) * np.power(lit(1.0, T) - cosine, lit(5.0, T))  # :96


def to_gamma(c):
    """:99-103."""
    T = c.dtype.type
    return np.power(c, T(f32(1.0) / f32(2.2)))


# ---------------------------------------------------------------------------
# geometry (:155-205)
# ---------------------------------------------------------------------------
def hit_world(spheres, o, d, t_min, t_max):
    """hit_world (:188-205) over hit_sphere (:155-186) for n rays: the spheres
    in order, each tried against the closest hit so far, the last accepted one
    kept. -> (hit (n,) bool, index (n,), t (n,), p (n, 3), normal (n, 3),
    front_face (n,) bool); the fields of a miss mean nothing."""
    T = o.dtype.type
    n = len(o)
    hit = np.zeros(n, bool)
    index = np.zeros(n, np.int64)
    closest = np.full(n, t_max, T)                                 # :192
    a = length(d) * length(d)                                      # :160
    with np.errstate(invalid="ignore", divide="ignore"):
        for i, s in enumerate(spheres):
            oc = o - s[:3]                                         # :159
            half_b = dot(oc, d)                                    # :161
            c = length(oc) * length(oc) - s[3] * s[3]              # :162
            disc = half_b * half_b - a * c                         # :164
            sq = np.sqrt(disc)                                     # :167 (NaN where :166 has returned)
            root = (-half_b - sq) / a                              # :170
            far = (root < t_min) | (closest < root)                # :171
            root = np.where(far, (-half_b + sq) / a, root)         # :173
            out = far & ((root < t_min) | (closest < root))        # :174
            ok = ~(disc < 0) & ~out                                # :166, :176
            hit |= ok                                              # :198
            closest = np.where(ok, root, closest)                  # :199
            index = np.where(ok, i, index)                         # :200
        won = spheres[index]
        p = o + col(closest) * d                                   # :181, :115
        outward = (p - won[:, :3]) / won[:, 3:4]                   # :182
        front = dot(d, outward) < 0                                # :145
    normal = np.where(col(front), outward, -outward)               # :146
    return hit, index, closest, p, normal, front


# ---------------------------------------------------------------------------
# scatter (:207-252), one function per branch
# ---------------------------------------------------------------------------
def scatter_diffuse(d, p, normal, values, seed):
    """:209-217 -> (direction, attenuation, seed, draws)."""
    rius, seed = random_in_unit_sphere(seed, d.dtype.type)
    target = p + normal + rius                                     # :211
    return normalize(target - p), values[:, :3], seed, 1           # :212, :215


def scatter_metal(d, p, normal, values, seed):
    """:219-227: the incoming direction as it is (not normalised), no test of
    which side the result points to (Appendix A 4)."""
    rius, seed = random_in_unit_sphere(seed, d.dtype.type)
    refl = reflect(d, normal)                                      # :221
    return normalize(refl + values[:, 3:4] * rius), values[:, :3], seed, 1  # :222, :225


def refraction_ratio(front, ir):
    """:232."""
    return np.where(front, lit(1.0, ir.dtype.type) / ir, ir)


def reflects(cant, refl, seed):
    """:241, `cant || reflectance > hash1(p)` without short circuit: hash1 is
    always drawn. -> (reflect?, seed, draws)."""
    h, seed = hash1(seed)
    return cant | (refl > h.astype(refl.dtype)), seed, 1


def scatter_dielectric(d, p, normal, front, values, seed):
    """:229-249."""
    T = d.dtype.type
    ratio = refraction_ratio(front, values[:, 3])
    unit = normalize(d)                                            # :234
    cosine = np.minimum(dot(-unit, normal), lit(1.0, T))           # :235
    sine = np.sqrt(lit(1.0, T) - cosine * cosine)                  # :236
    cant = ratio * sine > lit(1.0, T)                              # :238
    mirror, seed, draws = reflects(cant, reflectance(cosine, ratio), seed)
    direction = np.where(col(mirror), reflect(unit, normal), refract(unit, normal, ratio))  # :242, :244
    return direction, np.ones_like(d), seed, draws, mirror         # :231


def sky(d):
    """:279-281."""
    T = d.dtype.type
    t = lit(0.5, T) * (normalize(d)[:, 1] + lit(1.0, T))           # :280
    blue = np.array([lit(0.5, T), lit(0.7, T), lit(1.0, T)], T)
    return col(lit(1.0, T) - t) * np.ones(3, T) + col(t) * blue    # :281


def at_miss(before, now, sky_colour):
    """:283. `now` holds the attenuation of every hit so far (:269 runs before
    the next hit_world); `before` is `now` without the last hit's."""
    return now * sky_colour


# ---------------------------------------------------------------------------
# sample_color (:255-287) and the two entry points
# ---------------------------------------------------------------------------
class Tally:
    """What a batch of paths did, per path."""

    def __init__(self, n):
        self.segments = np.zeros(n, np.int64)   # hit_world calls
        self.draws = np.zeros(n, np.int64)      # hash1 / hash2 / hash3 calls
        self.reflections = np.zeros(n, np.int64)  # dielectric hits that took :242
        self.refractions = np.zeros(n, np.int64)  # ... and :244
        self.hits = np.zeros(n, np.int64)       # samples whose first segment hit something


def sample_color(spheres, mat_types, mat_values, o, d, seed, depth, tally):
    """:255-287 for n rays -> ((n, 3) colour, seed). seed: (n,) float32, read
    and returned; tally is added to."""
    T = o.dtype.type
    n = len(o)
    out = np.zeros((n, 3), T)                                      # :286 for whoever is still alive at the end
    now = np.ones((n, 3), T)                                       # :259
    before = np.ones((n, 3), T)
    o, d, seed = o.copy(), d.copy(), np.array(seed, f32)
    live = np.arange(n)
    for bounce in range(depth):                                    # :260
        if live.size == 0:
            break
        hit, index, _, p, normal, front = hit_world(spheres, o[live], d[live], lit(T_MIN, T), T(np.inf))  # :262
        tally.segments[live] += 1
        if bounce == 0:
            tally.hits[live[hit]] += 1
        miss = live[~hit]
        out[miss] = at_miss(before[miss], now[miss], sky(d[miss]))  # :279-283
        kind = mat_types[index]
        keep = np.zeros(live.size, bool)
        for code in (0, 1, 2):
            sel = hit & (kind == code)                             # :209, :219, :229
            if not sel.any():
                continue
            k, vals = live[sel], mat_values[index[sel]]
            if code == 0:
                nd, atten, seed[k], draws = scatter_diffuse(d[k], p[sel], normal[sel], vals, seed[k])
            elif code == 1:
                nd, atten, seed[k], draws = scatter_metal(d[k], p[sel], normal[sel], vals, seed[k])
            else:
                nd, atten, seed[k], draws, mirror = scatter_dielectric(d[k], p[sel], normal[sel], front[sel], vals,
                                                                       seed[k])
                tally.reflections[k] += mirror
                tally.refractions[k] += ~mirror
            tally.draws[k] += draws
            before[k] = now[k]
            now[k] = now[k] * atten                                # :269
            o[k], d[k] = p[sel], nd                                # :270
            keep |= sel
        # :251, :274: any other material code scatters nothing and the sample is black (out is 0 already)
        live = live[keep]
    return out, seed


def _as_T(a, dtype):
    return np.asarray(a, f32).astype(dtype)


def trace_batch(spheres, mat_types, mat_values, o, d, seed, samples, depth, dtype=np.float64):
    """What rays (o, d) see with the chains that start at `seed`: `samples`
    samples of sample_color each, every sample preceded by CSMain's two hash2
    draws (:306-307), whose values a path query has no use for (the contract of
    rtx_trace_paths: a query is a pixel of the frame whose film is a point).
    o, d: (n, 3) or (3,); seed: (n,); all float32 values.
    -> (sum (n, 3) dtype, end seed (n,) float32, Tally)."""
    seed = np.atleast_1d(np.asarray(seed, f32)).copy()
    n = len(seed)
    o = np.broadcast_to(_as_T(o, dtype), (n, 3))
    d = np.broadcast_to(_as_T(d, dtype), (n, 3))
    sph, mv = _as_T(spheres, dtype).reshape(-1, 4), _as_T(mat_values, dtype).reshape(-1, 4)
    mt = np.asarray(mat_types, f32).reshape(-1)
    total = np.zeros((n, 3), dtype)
    tally = Tally(n)
    for _ in range(samples):                                       # :304
        _, _, seed = hash2(seed)                                   # :306
        _, _, seed = hash2(seed)                                   # :307
        tally.draws += 2
        c, seed = sample_color(sph, mt, mv, o, d, seed, depth, tally)
        total = total + c                                          # :309
    return total, seed, tally


def trace(spheres, mat_types, mat_values, o, d, seed, samples, depth, dtype=np.float64):
    """One query of trace_batch -> (sum (3,), end seed, segments, draws)."""
    total, end, tally = trace_batch(spheres, mat_types, mat_values, o, d, [seed], samples, depth, dtype)
    return total[0], end[0], int(tally.segments[0]), int(tally.draws[0])


def jitter(x, y, seed, img_w, img_h):
    """:306-307 -> (u, v, seed): u from the first hash2's .x, v from the second
    hash2's .y."""
    T = img_w.dtype.type
    first_x, _, seed = hash2(seed)
    _, second_y, seed = hash2(seed)
    u = (x.astype(T) + first_x.astype(T) * lit(1.1, T)) / (img_w - lit(1.0, T))
    v = (y.astype(T) + second_y.astype(T) * lit(1.1, T)) / (img_h - lit(1.0, T))
    return u, v, seed


def get_ray(frame, u, v, dtype):
    """:118-127 with viewVals' rows = the frame's origin, horizontal,
    vertical, lower_left."""
    org, hor, ver, low = (_as_T(list(r)[:3], dtype) for r in (frame.origin, frame.horizontal, frame.vertical,
                                                              frame.lower_left))
    n = len(u)
    return np.broadcast_to(org, (n, 3)), low + col(u) * hor + col(v) * ver - org


def pixels(world, frame, xs, ys, dtype=np.float64):
    """CSMain (:292-315) for pixels (xs[i], ys[i]) of a pinhole, chain-RNG
    frame: -> (gamma colour (n, 3), segments (n,), end seed (n,))."""
    xs, ys = np.atleast_1d(np.asarray(xs, np.int64)), np.atleast_1d(np.asarray(ys, np.int64))
    img_w, img_h = np.asarray(f32(frame.img_w)).astype(dtype), np.asarray(f32(frame.img_h)).astype(dtype)  # :294
    seed = pixel_seed(xs, ys)                                      # :295
    sph, mv = _as_T(world.spheres, dtype).reshape(-1, 4), _as_T(world.mat_values, dtype).reshape(-1, 4)
    mt = np.asarray(world.mat_types, f32).reshape(-1)
    acc = np.zeros((len(xs), 3), dtype)                            # :303
    tally = Tally(len(xs))
    for _ in range(world.spp):                                     # :304
        u, v, seed = jitter(xs, ys, seed, img_w, img_h)
        o, d = get_ray(frame, u, v, dtype)
        c, seed = sample_color(sph, mt, mv, o, d, seed, world.depth, tally)
        acc = acc + c                                              # :309
    acc = acc / dtype(world.spp)                                   # :312
    with np.errstate(invalid="ignore"):
        return to_gamma(acc), tally.segments, seed                 # :313


def pixel(world, frame, x, y, dtype=np.float64):
    c, s, seed = pixels(world, frame, [x], [y], dtype)
    return c[0], int(s[0]), seed[0]
