# Objects of the reference's own binding glue (bindings/python/ckzg_wrap.c, bindings/csharp/ckzg_wrap.c), compiled
# unchanged against include/ckzg.h into oracle/_ref/ (kept out of git) for tests/test_reference_bindings_link.py.
# build() runs this only where the reference tree exists:  make -f ref.mk REFERENCE=<tree> PYINC=<Python.h dir>
CC ?= gcc
REFERENCE ?=
PYINC ?=
OUT = _ref
INC = -I../include
all: $(OUT)/ckzg_cs_wrap.o $(if $(PYINC),$(OUT)/ckzg_py_wrap.o)
$(OUT)/ckzg_cs_wrap.o: $(REFERENCE)/bindings/csharp/ckzg_wrap.c ../include/ckzg.h
	@mkdir -p $(OUT)
	$(CC) -O1 -fPIC $(INC) -I$(REFERENCE)/bindings/csharp -c $< -o $@
$(OUT)/ckzg_py_wrap.o: $(REFERENCE)/bindings/python/ckzg_wrap.c ../include/ckzg.h
	@mkdir -p $(OUT)
	$(CC) -O1 -fPIC $(INC) -I$(PYINC) -c $< -o $@
clean:
	rm -rf $(OUT)
.PHONY: all clean
