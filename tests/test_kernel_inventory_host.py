"""CPU: tests/kernel_inventory.py names every kernel of csrc/ and nothing else, every test file it names mentions the entry it names, and
none of the nine small kernels of tests/test_gpu_tokens.py has gone back to being reached through whole forwards only.  Names only: no
generated code is looked at."""
import glob
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kernel_inventory as K  # noqa: E402
import tokens_ref as T  # noqa: E402

TESTS = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(TESTS), "anime-illust-image-searcher_amd", "csrc")
KERNEL = re.compile(r"__global__[^;{]*?\bvoid\s+(\w+)\s*\(")


def _strip_comments(text):
    return re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S)


def kernels_in_sources():
    names = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))):
        text = _strip_comments(open(path).read())
        found = KERNEL.findall(text)
        assert len(found) == text.count("__global__"), "%s: a __global__ the pattern does not read" % os.path.basename(path)
        for name in found:
            names.setdefault(name, []).append(os.path.basename(path))
    return names


def test_every_kernel_is_in_the_table_and_the_table_names_no_other():
    names = kernels_in_sources()
    assert len(names) > 80
    assert sorted(n for n in names if n not in K.KERNEL_TESTS) == [], "kernels without an entry in tests/kernel_inventory.py"
    assert sorted(n for n in K.KERNEL_TESTS if n not in names) == [], "entries for kernels that are gone"


def test_named_test_files_mention_the_named_entries():
    for kernel, (where, what) in K.KERNEL_TESTS.items():
        assert isinstance(what, str) and what, kernel
        if where == K.FORWARD_ONLY:
            assert len(what) > 20, "%s: a reason, please" % kernel
            continue
        path = os.path.join(TESTS, where)
        assert os.path.isfile(path), "%s: %s does not exist" % (kernel, where)
        assert re.search(r"\b%s\b" % re.escape(what), open(path).read()), "%s: %s does not mention %s" % (kernel, where, what)


def test_the_token_kernels_are_tested_on_their_own():
    assert len(T.TOKEN_KERNELS) == 9
    for kernel in T.TOKEN_KERNELS:
        where, what = K.KERNEL_TESTS[kernel]
        assert where == "test_gpu_tokens.py" and what.startswith("hiptsdbg_"), kernel
