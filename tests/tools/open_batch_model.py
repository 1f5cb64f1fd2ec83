"""CPU model of the batched calls of bbg_open_all (bbg_open_all_batch*, csrc/open_all.hip, csrc/ecntt.hip), on Python integers mod r: any
abelian group shows whether a schedule or an index is right, and Fr is the one at hand.

    batched_stages       what ecntt_stages_batch queues: the log2block radix-2 stages of the 2^log2block domain, each ONE pass whose
                         butterfly index t runs to count 2^(log2block - 1) over `count` contiguous blocks; i = (t >> s << (s + 1)) + j with
                         j = t mod 2^s, the twiddle w^(+-j 2^(log2block - 1 - s)) from j alone, and in the inverse direction n^-1 folded into
                         the last stage (both operands), as k_ecntt_stage does.  Blocks bit-reversed within themselves in, natural order out.
    transform            one block's transform by its definition, the thing the above must equal block by block.
    lds_transform        k_open_batch_ntt_lds on one block: bit-reversed load, the same stages, natural order out.
    product_destination  where k_open_batch_pointwise writes product (p, b, i): item g = p 2n + b 2r + i goes to (g - q) + bitrev_2n(q),
                         q = g mod 2n.
    fold_source          where k_open_all_fold reads entry i of polynomial p.
    chunk_walk           the chunks open_all_batch_run walks: (first polynomial, polynomials) under a reservation of `cap`.
    batch_cap            the polynomials one workspace may hold under the budget, from the single call's byte formula."""
import coarse_inputs as ci
import open_all_model as oa
import open_cells_model as oc

R_MOD = oa.R_MOD
BUDGET = 1 << 30  # OPEN_BATCH_BUDGET (csrc/open_all.hip)
LDS_LOG2 = 12     # OPEN_BATCH_LDS_LOG2: the largest 2r = 2^12 the LDS transform takes


def transform(vals, inverse=False):
    """out[k] = sum_j vals[j] w^(jk), or n^-1 sum_j vals[j] w^(-jk), w the root of the len(vals) domain."""
    n = len(vals)
    w = ci.root_of_unity(n.bit_length() - 1)
    if not inverse:
        return oa.fr_ntt(vals, w)
    n_inv = pow(n, R_MOD - 2, R_MOD)
    return [v * n_inv % R_MOD for v in oa.fr_ntt(vals, pow(w, R_MOD - 2, R_MOD))]


def batched_stages(work, log2block, count, inverse=False):
    """In: count blocks of 2^log2block values, each bit-reversed within itself.  Out: every block transformed, natural order."""
    work = list(work)
    n = 1 << log2block
    assert len(work) == count * n and log2block >= 1
    w = ci.root_of_unity(log2block)
    if inverse:
        w = pow(w, R_MOD - 2, R_MOD)
    n_inv = pow(n, R_MOD - 2, R_MOD)
    for s in range(log2block):
        m = 1 << s
        last = inverse and s + 1 == log2block
        for t in range(count << (log2block - 1)):  # one launch
            j = t & (m - 1)
            i = ((t >> s) << (s + 1)) + j
            tw = pow(w, j << (log2block - 1 - s), R_MOD)
            a, b = work[i], work[i + m]
            if last:
                tw, a = tw * n_inv % R_MOD, a * n_inv % R_MOD
            b = b * tw % R_MOD
            work[i], work[i + m] = (a + b) % R_MOD, (a - b) % R_MOD
    return work


def bit_reversed_blocks(vals, log2block):
    n = 1 << log2block
    return [vals[(k // n) * n + oc.bit_reverse(k % n, log2block)] for k in range(len(vals))]


def lds_transform(vals):
    log2b = len(vals).bit_length() - 1
    return batched_stages(bit_reversed_blocks(vals, log2b), log2b, 1)


def product_destination(p, b, i, log2n, log2cell):
    log2m = log2n + 1
    g = (p << log2m) + (b << (log2m - log2cell)) + i
    q = g & ((1 << log2m) - 1)
    return (g - q) + oc.bit_reverse(q, log2m)


def fold_source(p, i, log2p):
    g = (p << log2p) + i
    return ((g - i) << 1) + oc.bit_reverse(i, log2p)


def chunk_walk(count, cap):
    out, done = [], 0
    while done < count:
        c = min(cap, count - done)
        out.append((done, c))
        done += cap
    return out


def handle_bytes(log2n, log2cell):
    """bbg_open_all_device_bytes of a handle that holds no batch workspace."""
    n = 1 << log2n
    r = n >> log2cell
    if log2cell == 0:
        return 2 * n * 64 + 2 * n * 128 + n * 128 + 2 * n * 32
    return 2 * n * 64 + 2 * n * 128 + 2 * n * 32 + 2 * r * 128 + r * 128


def poly_bytes(log2n, log2cell):
    """The workspace of one polynomial: the handle's buffers without the 2n transformed points."""
    return handle_bytes(log2n, log2cell) - 2 * (1 << log2n) * 64


def batch_cap(log2n, log2cell):
    return max(1, BUDGET // poly_bytes(log2n, log2cell))
