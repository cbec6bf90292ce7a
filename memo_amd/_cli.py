"""The frame every sub-command of bin/memo beyond `query` and `index` stands in: usage, refusals, the flags, the device, the
error tail and the output file.

A memo_amd/NAME_cli.py fills a Cli with its name, its USAGE, its getopt string and its defaults, and its main() reads top to
bottom as what is particular to the sub-command.  The conventions are the reference's shell front ends': a bad flag gets bash
getopts' message on stderr, then the usage, exit 0; a missing required flag exits 2 (argparse's status); everything that can be
refused is refused, as `memo NAME: ...` on stderr with status 1, before the device is touched; an output file is whole or it is not
there.
"""
import getopt
import os
import sys


class Cli:
    def __init__(self, name, usage_text, optstring, defaults=None, banner=None):
        self.name, self.usage_text, self.optstring = name, usage_text, optstring
        self.defaults = dict(defaults or {})
        self.banner_text = f"MEMO - {name}" if banner is None else banner

    def usage(self):
        sys.stdout.write(self.usage_text)
        sys.exit(0)

    def refuse(self, message, status=1):
        sys.stderr.write(f"memo {self.name}: {message}\n")
        sys.exit(status)

    def options(self, argv):
        """getopt's (flag, value) pairs in command order; no argument, -h or a flag getopt refuses ends in the usage"""
        if not argv or argv[0] == "-h":
            self.usage()
        try:
            return getopt.getopt(argv, self.optstring)[0]
        except getopt.GetoptError as exc:
            what = "option requires an argument" if "requires argument" in exc.msg else "illegal option"
            sys.stderr.write(f"{sys.argv[0]}: {what} -- {exc.opt}\n")
            self.usage()

    def banner(self):
        print(self.banner_text, flush=True)

    def parse(self, argv):
        """{flag: value} over the defaults (the last of a repeated flag holds), and the banner"""
        val = dict(self.defaults)
        val.update(self.options(argv))
        self.banner()
        return val

    def require(self, val, flags):
        missing = [f for f in flags if val.get(f, "") == ""]
        if missing:
            self.refuse(f"{', '.join(missing)} required", 2)

    def one_gpu_only(self):
        if sharded_launch():
            self.refuse("one GPU only: a sharded launch (WORLD_SIZE > 1, MEMO_FORCE_SHARDED) is not supported")

    def integers(self, val, *flags):
        """int() of each flag's value; what int() says about one that is none is the refusal"""
        try:
            return [int(val[f]) for f in flags]
        except ValueError as exc:
            self.refuse(str(exc))

    def integer(self, flag, text, lo, hi, what):
        """an integer of [lo, hi], which the refusal spells as `what`"""
        try:
            value = int(text)
        except ValueError:
            value = lo - 1
        if not lo <= value <= hi:
            self.refuse(f"{flag} must be an integer in {what} (got {text!r})")
        return value

    def guarded(self, fn):
        """fn(), the part that touches files and the device.  What a user can cause is a refusal: a window or a file that is
        refused (pyarrow's errors are ValueErrors and OSErrors), a device call that fails, the sweep's own IndexError
        (index.check), a record that is not there.  Anything else is a defect and leaves as a traceback, as from `memo query`."""
        from ._lib import MemoError
        try:
            return fn()
        except (MemoError, OSError, LookupError, ValueError) as exc:
            self.refuse(f"{type(exc).__name__}: {exc}" if isinstance(exc, LookupError) else str(exc))

    def read_labels(self, path, n_docs):
        """the labels of the genome list `memo index -g` took, one per genome, the pivot first"""
        try:
            with open(path) as fh:
                lines = [ln.strip() for ln in fh if ln.strip()]
        except OSError as exc:
            self.refuse(f"cannot read the genome list {path}: {exc.strerror}")
        if len(lines) != n_docs:
            self.refuse(f"-g {path} names {len(lines)} genomes, -n says {n_docs}")
        return [label_of(ln) for ln in lines]


def sharded_launch():
    return int(os.environ.get("WORLD_SIZE", "1") or "1") > 1 or bool(os.environ.get("MEMO_FORCE_SHARDED"))


def device():
    """as `memo query` chooses its GPU"""
    return int(os.environ.get("MEMO_DEVICE", "0"))


def label_of(path):
    """a genome's label: its file's base name without extension (a trailing .gz goes first: g1.fa.gz and g1.fa are both g1)"""
    name = os.path.basename(path.strip())
    if name.endswith(".gz"):
        name = name[:-3]
    return os.path.splitext(name)[0]


def replace_into(path, write):
    """write(tmp) and then rename: the file is whole or it is not there"""
    tmp = f"{path}.part{os.getpid()}"
    try:
        write(tmp)
        os.replace(tmp, path)
    except BaseException:
        if os.path.exists(tmp):
            os.unlink(tmp)
        raise


def replace_all_into(paths, write):
    """write([tmp, ...]), one beside every path, and then rename from the last to the first: no file is replaced before all are
    whole, and nothing is left behind"""
    def nest(at, tmps):
        if at == len(paths):
            write(tmps)
        else:
            replace_into(paths[at], lambda tmp: nest(at + 1, tmps + [tmp]))
    nest(0, [])


def _write(path, mode, data):
    def write(tmp):
        with open(tmp, mode) as fh:
            fh.write(data)
    replace_into(path, write)


def write_text(path, text):
    _write(path, "w", text)


def write_bytes(path, buf):
    """buf: bytes, or a uint8 array as the emit functions return it"""
    _write(path, "wb", memoryview(buf))
