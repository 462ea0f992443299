"""decoding.shared_prefix_len: the number of leading spliced positions that B prompts about one picture share (pure host code)."""
import pytest

IMG = -200  # constants.IMAGE_TOKEN_INDEX: stands for the 256 image feature rows
SYSTEM = list(range(1000, 1036))  # 36 ids before the image, as the llava_v1 system text


def _prompt(tail, head=SYSTEM):
    return list(head) + [IMG] + list(tail)


def test_identical_prompts_share_all_but_the_last_row():
    from interactvlm_amd.decoding import shared_prefix_len

    p = _prompt(range(40, 60))
    T0 = len(p) - 1 + 256
    # (B identical prompts leave B suffix rows, one each: 17 of them make the packed suffix pass a tile GEMM, M > 16)
    assert shared_prefix_len([p] * 17, True) == T0 - 1
    assert shared_prefix_len([p] * 16, True) == 0  # 16 suffix rows in all: the plain path


def test_prompts_that_differ_after_the_image():
    from interactvlm_amd.decoding import shared_prefix_len

    common = [7, 8, 9, 10, 11]
    prompts = [_prompt(common + [50 + b] * (9 + b)) for b in range(3)]  # different tails of different lengths
    assert shared_prefix_len(prompts, True) == 36 + 256 + len(common)
    # the cap: a prompt that is a proper prefix of the others keeps its last row for itself
    short = _prompt(common)
    assert shared_prefix_len([short] + prompts, True) == 36 + 256 + len(common) - 1
    # another image length (the toy towers)
    assert shared_prefix_len(prompts, True, image_rows=16) == 36 + 16 + len(common)


def test_a_difference_before_the_image_gives_its_index():
    from interactvlm_amd.decoding import shared_prefix_len

    a, b = list(SYSTEM), list(SYSTEM)
    b[20] = 5
    tail = list(range(40, 60))
    assert shared_prefix_len([_prompt(tail, a), _prompt(tail, b)], True) == 20
    b = list(SYSTEM)
    b[16] = 5  # 16 shared rows: too few for the tile GEMMs
    assert shared_prefix_len([_prompt(tail, a), _prompt(tail, b)], True) == 0
    b = list(SYSTEM)
    b[17] = 5
    assert shared_prefix_len([_prompt(tail, a), _prompt(tail, b)], True) == 17


def test_nothing_shared_takes_the_plain_path():
    from interactvlm_amd.decoding import shared_prefix_len

    prompts = [_prompt([7, 8, 9] + [50 + b] * 12) for b in range(3)]
    assert shared_prefix_len(prompts, True) == 36 + 256 + 3
    assert shared_prefix_len(prompts, False) == 0  # several pictures
    assert shared_prefix_len(prompts[:1], True) == 0  # B = 1
    assert shared_prefix_len([[1, 2, 3, 4] + [9] * 30, [1, 2, 3, 4] + [8] * 30], True) == 0  # P <= 16
    assert shared_prefix_len([_prompt([7] * 8 + [1]), _prompt([7] * 8 + [2])], True) == 0  # 2 suffix rows


@pytest.mark.parametrize("mode", ["default", "bf16", "parity", "parity-fast"])
def test_modes(mode):
    from interactvlm_amd.decoding import SHARED_PREFIX_MODES, shared_prefix_len

    prompts = [_prompt([7, 8, 9] + [50 + b] * 12) for b in range(3)]
    assert SHARED_PREFIX_MODES == ("default", "bf16")
    assert shared_prefix_len(prompts, True, mode) == (36 + 256 + 3 if mode in ("default", "bf16") else 0)
    assert shared_prefix_len(prompts, True, mode, fp8=True) == 0


def test_public_keywords_exist():
    import inspect

    from interactvlm_amd import llava, model

    for fn in (model.InteractVLMForCausalLM.generate_batch, model.InteractVLMForCausalLM.evaluate_batch):
        assert inspect.signature(fn).parameters["share_prefix"].default is False
    assert inspect.signature(llava.Llama.decode_step_batch).parameters["prefix"].default is None
    K = llava._GraphKey
    assert K(True, 2, "f16", True, False, False) == K(True, 2, "f16", True, False, False, False, False)  # existing keys compare as before
    assert K(True, 2, "f16", True, False, False) != K(True, 2, "f16", True, False, False, prefix=True)
