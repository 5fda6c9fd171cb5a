"""What the ABI tests (tests/test_*abi.py) read out of the public headers under include/: the declared functions, the
values of an enum and the members of a struct."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_text(header="sfgpu.h"):
    return open(os.path.join(ROOT, "include", header)).read()


def declared_functions(header):
    text = header_text(header)
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    return sorted(set(re.findall(r"\b(?:int|void|const char\s*\*)\s+(\w+)\s*\(", text)))


def enum_values(header_text, enum_name):
    """{name: value as written} of `enum enum_name { SF_X = 0, ... }`."""
    m = re.search(r"enum\s+%s\s*\{([^}]*)\}" % enum_name, header_text)
    assert m, f"the header does not declare enum {enum_name}"
    return dict(re.findall(r"(SF_\w+)\s*=\s*(\d+)", m.group(1)))


def struct_members(header_text, struct_name):
    """[(member, C type)] of `typedef struct struct_name { ... } struct_name;`, in order."""
    m = re.search(r"typedef\s+struct\s+%s\s*\{([^}]*)\}\s*%s\s*;" % (struct_name, struct_name), header_text)
    assert m, f"the header does not declare struct {struct_name}"
    members = []
    for decl in m.group(1).split(";"):
        decl = " ".join(decl.split())
        if not decl:
            continue
        ctype = "long long" if decl.startswith("long long ") else decl.split(" ")[0]
        members += [(n.strip(), ctype) for n in decl[len(ctype):].split(",")]
    return members


def struct_field_names(header_text, struct_name):
    return [n for n, _ in struct_members(header_text, struct_name)]
